"""The decode launch plan (csrc/awq_decode_plan.hpp: which kernel, which row chunks, which configuration) on the host, no GPU:

  * the library's two queries answer the pinned table of tests/decode_plan_cases.py word for word;
  * the knobs that were frozen are refused, the ones that stay change the words they are meant to change and nothing else;
  * the header alone, in a stand-alone program built with the host compiler under AddressSanitizer and UBSan, keeps the invariants
    launch_gemv_dma relies on over the whole grid (tests/decode_plan_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import decode_plan_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELETED = ("gemvd_four", "gemvd_wide8", "decode_skinny_small", "decode_skinny_m1", "skinny_deep64", "skinny_xu", "gemvd_bpc", "gemvd_ns2")
DEFAULTS = dict(decode_skinny_from=0, gemvd_waves=0, gemvd_d=0, gemvd_want=0, gemvd_il=2, gemvd_probe=0)


def _lib():
    from llm_awq_amd import _capi
    return _capi, _capi.lib()


def _plan(L, m, n, k, epi):
    kern = ctypes.c_int(-1)
    passes = L.awq_w4a16_decode_cdna4_plan(m, n, k, epi, ctypes.byref(kern))
    out = (ctypes.c_int * 8)()
    count = L.awq_w4a16_decode_cdna4_plan_detail(m, n, k, epi, 0, out)
    chunks = []
    for i in range(count):
        assert L.awq_w4a16_decode_cdna4_plan_detail(m, n, k, epi, i, out) == count
        chunks.append(tuple(out))
    return passes, kern.value, tuple(chunks)


@pytest.fixture
def tuned():
    capi, L = _lib()
    capi.tune(**DEFAULTS)
    yield capi, L
    capi.tune(**DEFAULTS)


def test_the_table_covers_the_shapes_and_the_class_edges():
    keys = {(epi, m, n, k) for epi, m, n, k, *_ in C.CASES}
    for n, k, epis in [(6144, 4096, (0,)), (4096, 4096, (0,)), (28672, 4096, (1, 2)), (4096, 14336, (0,)), (10240, 8192, (0,)), (8192, 8192, (0,)),
                       (57344, 8192, (1, 2)), (8192, 28672, (0,)), (12288, 4096, (0,)), (4096, 11008, (0,)), (768, 768, (0,)), (3072, 768, (0,)), (768, 3072, (0,))]:
        for epi in epis:
            for m in range(1, 9):
                assert (epi, m, n, k) in keys, (epi, m, n, k)
    for slabs in (256, 257, 383, 384, 512, 513, 768, 769, 1023, 1024):
        for nit in (31, 32, 63, 64, 95, 96, 112):
            for m in (1, 2, 4, 5, 8):
                assert (0, m, 16 * slabs, 128 * nit) in keys and (1, m, 32 * slabs, 128 * nit) in keys, (m, slabs, nit)


def test_both_queries_answer_the_pinned_table(tuned):
    _, L = tuned
    wrong = [(case, got) for case in C.CASES for got in [_plan(L, case[1], case[2], case[3], case[0])] if got != tuple(case[4:])]
    assert not wrong, (len(wrong), wrong[:5])
    for epi, m, n, k, passes, kernel, chunks in C.CASES:   # the table itself: one answer of the old query per plan
        assert passes == len(chunks) and sum(c[0] for c in chunks) == m and kernel == int(len(chunks) == 1 and chunks[0][1] == 1)


def test_detail_query_edges(tuned):
    _, L = tuned
    out = (ctypes.c_int * 8)(*([-5] * 8))
    assert L.awq_w4a16_decode_cdna4_plan_detail(7, 4096, 14336, 0, 0, None) == 1          # out may be NULL
    assert L.awq_w4a16_decode_cdna4_plan_detail(7, 4096, 14336, 0, 1, out) == 1 and list(out) == [-5] * 8   # no such chunk: untouched
    assert L.awq_w4a16_decode_cdna4_plan_detail(7, 4096, 14336, 0, -1, out) == 1 and list(out) == [-5] * 8
    for m, n, k, epi in [(9, 4096, 4096, 0), (0, 4096, 4096, 0), (4, 4100, 4096, 0), (4, 4096, 4000, 0), (4, 4112, 4096, 1), (4, 4096, 4096, 3)]:
        assert L.awq_w4a16_decode_cdna4_plan_detail(m, n, k, epi, 0, out) == 0 and list(out) == [-5] * 8, (m, n, k, epi)


def test_frozen_knobs_are_refused(tuned):
    capi, L = tuned
    for key in DELETED:
        assert L.awq_tune_set(key.encode(), 1) == -4, key   # AWQ_ERR_SHAPE, as any unknown key
    assert L.awq_tune_set(b"no_such_knob", 1) == -4


def test_kept_knobs_change_the_words_they_should(tuned):
    capi, L = tuned
    o_proj, down, gate_up = (4096, 4096, 0), (4096, 14336, 0), (28672, 4096, 2)
    base = {(m, s): _plan(L, m, *s) for m in (1, 4, 7) for s in (o_proj, down, gate_up)}
    assert base[1, o_proj] == (1, 0, ((1, 0, 8, 4, 2, 26752, 3, 0),))

    capi.tune(decode_skinny_from=9)   # never the skinny kernel: every chunk streaming, K = 14336 at seven rows in chunks that sum to seven
    for (m, s), _ in base.items():
        passes, kernel, chunks = _plan(L, m, *s)
        assert kernel == 0 and passes == len(chunks) and all(c[1] == 0 and c[7] == 0 for c in chunks) and sum(c[0] for c in chunks) == m
    assert _plan(L, 7, *down)[0] >= 2
    capi.tune(decode_skinny_from=1)   # always: one skinny launch, streaming words zero, shape and pieces as at the default
    assert _plan(L, 1, *o_proj) == (1, 1, ((1, 1, 0, 0, 0, 0, 0, 8 * 1 + 1),)) and _plan(L, 7, *gate_up) == base[7, gate_up]
    assert _plan(L, 1, 28672, 4096, 1)[1] == 0   # (the stacked epilogue has no skinny form, whatever the knob says)
    capi.tune(decode_skinny_from=5)
    assert [_plan(L, m, *o_proj)[1] for m in (4, 5)] == [0, 1]
    capi.tune(decode_skinny_from=0)

    for waves, d in [(4, 4), (8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4)]:   # forced pairs: waves and ring depth, nothing else but what follows from them
        capi.tune(gemvd_waves=waves, gemvd_d=d)
        passes, kernel, ((rows, kern, w, tx, dd, smem, flags, sk),) = _plan(L, 1, *o_proj)
        assert (passes, kernel, rows, kern, sk) == (1, 0, 1, 0, 0) and w == waves and tx == 32 // waves and dd == min(d, tx), (waves, d)
        txp = (tx + 3) & ~3
        assert smem == waves * (dd * 1024 + txp * 64 + txp * 256 + 16)   # ring + scales + one row of x per wave
        assert flags & 1 == int(waves == 8 and dd < tx) and flags >> 1 == int((waves, dd, tx) in ((8, 2, 4), (8, 4, 4)))
    capi.tune(gemvd_waves=0, gemvd_d=0)

    capi.tune(gemvd_il=0)   # bit 0 of the flags, and only that
    p = _plan(L, 1, *o_proj)
    assert p[2][0][6] == 2 and p[2][0][:6] == base[1, o_proj][2][0][:6]
    capi.tune(gemvd_il=1)
    p = _plan(L, 1, *down)
    assert p[2][0][6] == 3 and p[2][0][:6] == base[1, down][2][0][:6] and base[1, down][2][0][6] == 2
    capi.tune(gemvd_il=2)

    capi.tune(gemvd_want=1)   # the LDS budget of ONE block per CU: a deeper ring on the gate/up pair at four rows, the same waves and steps
    p, b = _plan(L, 4, *gate_up)[2][0], base[4, gate_up][2][0]
    assert p[:4] == b[:4] and p[4] > b[4] and p[5] > b[5]
    capi.tune(gemvd_want=0)

    capi.tune(gemvd_probe=3)  # no rule reads the probes
    assert all(_plan(L, m, *s) == v for (m, s), v in base.items())
    capi.tune(gemvd_probe=0)
    assert all(_plan(L, m, *s) == v for (m, s), v in base.items())


def test_header_alone_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "decode_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "llm_awq_amd", "csrc"), os.path.join(ROOT, "tests", "decode_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe, "32"], capture_output=True, text=True, timeout=600)   # (no argument: every slab count, about a minute)
    assert r.returncode == 0 and r.stdout.strip().endswith(" 0 failures"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
