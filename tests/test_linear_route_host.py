"""The route of the dense W4 cdna4 linear entries (csrc/awq_linear_route.hpp: which ONE launcher serves a call) on the host, no GPU:

  * awq_w4a16_linear_route_cdna4 and the two workspace queries answer the pinned table of tests/linear_route_cases.py word for word, at the
    defaults and at every knob block;
  * the header alone, in a stand-alone program built with the host compiler under AddressSanitizer and UBSan, keeps the invariants the entries
    rely on when they switch on a route without falling through (tests/linear_route_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import linear_route_cases as C
from tools import linear_route_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def tuned():
    from llm_awq_amd import _capi
    _capi.tune(**G.DEFAULTS)
    yield _capi, _capi.lib()
    _capi.tune(**G.DEFAULTS)


def test_the_table_covers_the_shapes_and_the_class_edges():
    lines = {(b, e, n, k): per_m for b, e, n, k, per_m in C.CASES}
    assert all(len(per_m) == len(G.ROWS) == 20 for per_m in lines.values()) and all(len(p) == 32 for p in C.PATTERNS)   # every row count, every combination of the flags
    assert set(G.ROWS) == {1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 71, 72, 128, 129, 192, 255, 256, 300, 2048}
    for e in range(6):   # all six entries at the defaults: the model shapes, then slab counts x k-steps at the edges midm_small_takes and seven_slab_round read
        for n, k in [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672), (12288, 4096),
                     (22016, 4096), (4096, 11008), (768, 768), (3072, 768), (768, 3072)]:
            assert (0, e, n, k) in lines, (e, n, k)
        for slabs in (511, 512, 639, 640, 1023, 1024):
            for nit in (191, 192):
                assert (0, e, 16 * slabs, 128 * nit) in lines, (e, slabs, nit)
        assert (0, e, 16368, 128 * 192) in lines and (0, e, 16384, 128 * 192) in lines
    blocks = G.blocks()   # one block of rows for each non-default knob value that a test of the suite sets
    assert [b for b, _ in blocks[1:]] == [dict(midm=0), dict(midm_min=9, midm_max=255), dict(midm_max=192), dict(gemm_small_m=0), dict(gemm_small_m=2)] + \
        [dict(gemm_variant=v) for v in (1, 2, 3, 4, 5)] + [dict(mlp_skinny_max=8), dict(skinny16_szh=0), dict(gemv_dma=0)]
    for b in range(1, len(blocks)):
        assert all((b, e, n, k) in lines for e in range(6) for n, k in G.KNOB_SHAPES), b
    assert len(lines) == len(C.CASES) == sum(6 * len(shapes) for _, shapes in blocks)
    assert {(b, n, k) for b, n, k, *_ in C.WORKSPACE} == {(b, n, k) for b, _, n, k in lines}
    used = {c for per_m in lines.values() for p in per_m for c in C.PATTERNS[p]}
    assert used == set(C.WORDS) | {"."} and {w[0] for w in C.WORDS.values()} == set(range(1, 9))   # every leaf occurs


def test_the_queries_answer_the_pinned_table(tuned):
    capi, L = tuned
    wrong, compared, now = [], 0, None
    for b, e, n, k, per_m in C.CASES:   # (the table is in block order: each block's knobs are set once)
        if b != now:
            capi.tune(**{**G.DEFAULTS, **G.blocks()[b][0]})
            now = b
            for wb, wn, wk, fwd, pair in C.WORKSPACE:
                if wb == b and (fwd, pair) != G.workspace(L, wn, wk):
                    wrong.append(("workspace", b, wn, wk, G.workspace(L, wn, wk)))
        for m, p, got in zip(G.ROWS, per_m, G.answers(L, e, n, k)):
            want = tuple(C.WORDS.get(c, ()) for c in C.PATTERNS[p])
            compared += 32
            if got != want:
                wrong.append((b, e, m, n, k, [(f, g, w) for f, (g, w) in enumerate(zip(got, want)) if g != w][:3]))
    assert not wrong, (len(wrong), wrong[:5])
    assert compared == len(C.CASES) * 20 * 32


def test_query_edges(tuned):
    _, L = tuned
    out = (ctypes.c_int * 8)(*([-5] * 8))
    assert L.awq_w4a16_linear_route_cdna4(0, 100, 4096, 4096, 13, None) == 3   # out may be NULL
    for entry, m, n, k, flags in [(-1, 1, 4096, 4096, 1), (6, 1, 4096, 4096, 1), (0, 0, 4096, 4096, 1), (0, 1, 4104, 4096, 1), (0, 1, 8, 4096, 1), (0, 1, 4096, 4000, 1),
                                  (0, 1, 4096, 0, 1), (0, 1, 4096, 4096, 32), (0, 1, 4096, 4096, -1), (3, 17, 4096, 4096, 1), (4, 1, 4096, 4096, 0), (5, 1, 4096, 4096, 2),
                                  (4, 300000, 4096, 8192, 1)]:
        assert L.awq_w4a16_linear_route_cdna4(entry, m, n, k, flags, out) == 0 and list(out) == [-5] * 8, (entry, m, n, k, flags)


def test_header_alone_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "linear_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "llm_awq_amd", "csrc"), os.path.join(ROOT, "tests", "linear_route_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith(" 0 failures"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
