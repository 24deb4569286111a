"""Prompt chunks on the device-length and paged KV caches, without a GPU: the four exports at every layer, every argument check of the C ABI,
the module's and the shim's routing, and the soundness of the needle batches of tests/attn_prefill_kvcache_cases.py -- the lists
tests/test_gpu_attention_prefill_kvcache.py runs through the kernels -- against the float64 restatement of the calls and each of its
mutants."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_kvcache_cases as C

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
SYMBOLS = ("awq_attn_prefill_kvcache", "awq_attn_prefill_kvcache_kv8", "awq_attn_prefill_paged", "awq_attn_prefill_paged_kv8")
LL, I, VP, F = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float


def bits(t):
    return t.view(torch.int16)


def test_library_engine_and_ops_export_the_prefill_kvcache_surface():
    L = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    # the argument order of the attn_kvcache* neighbours
    for new, old in (("attn_prefill_kvcache", "attn_kvcache"), ("attn_prefill_kvcache_kv8", "attn_kvcache_kv8"),
                     ("attn_prefill_paged", "attn_kvcache_paged"), ("attn_prefill_paged_kv8", "attn_kvcache_paged_kv8")):
        assert params(getattr(eng, new)) == params(getattr(eng, old)), new
    assert params(eng.attn_prefill_paged_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table", "seqlens_k", "max_seqlen_k",
                                                  "seqlen_offset", "softmax_scale", "causal"]
    assert list(inspect.signature(ops.attn_prefill_kvcache).parameters) == list(inspect.signature(ops.attn_kvcache).parameters) == [
        "q", "k_cache", "v_cache", "seqlens_k", "max_seqlen_k", "seqlen_offset", "softmax_scale", "causal", "k_scale", "v_scale"]
    assert list(inspect.signature(ops.attn_prefill_paged).parameters) == list(inspect.signature(ops.attn_kvcache_paged).parameters)


def test_capi_signatures_are_the_kvcache_entries_without_the_workspace():
    S = _capi.SIGNATURES
    for new, old in (("awq_attn_prefill_kvcache", "awq_attn_kvcache"), ("awq_attn_prefill_kvcache_kv8", "awq_attn_kvcache_kv8"),
                     ("awq_attn_prefill_paged", "awq_attn_kvcache_paged"), ("awq_attn_prefill_paged_kv8", "awq_attn_kvcache_paged_kv8")):
        res, args = S[new]
        ores, oargs = S[old]
        assert res is I is ores
        assert oargs[-3:] == [VP, ctypes.c_size_t, VP] and args == oargs[:-3] + [VP], new   # workspace and its size are gone, the stream stays
    assert S["awq_attn_prefill_kvcache"][1] == [VP] * 4 + [I, I, VP] + [I] * 6 + [LL] * 6 + [F, I, I, VP]
    assert S["awq_attn_prefill_paged_kv8"][1] == [VP] * 7 + [I, I, VP] + [I] * 5 + [LL] + [I] * 3 + [LL] * 10 + [F, I, I, VP]


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call.  There is no workspace to withhold, so a call that passed every check would launch: every
# call here is refused, and a shape is shown to PASS the shape phase by the code of a later phase (alignment).
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


DENSE_OK = dict(B=2, Sq=512, off=512, bound=4096, lmax=4100, H=8, Hkv=2, Dh=128, qbs=512 * 1024, qrs=1024, kbs=4100 * 256, krs=256, vbs=4100 * 256,
                vrs=256, ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0)
PAGED_OK = dict(B=2, Sq=512, off=512, bound=4096, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qbs=512 * 1024, qrs=1024, kps=256 * 256,
                krs=256, vps=256 * 256, vrs=256, ksps=256 * 2, ksrs=2, vsps=256 * 2, vsrs=2, scale=0.1, causal=1, dtype=0)


def _dense(p, kv8=False, **kw):
    a = dict(DENSE_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, lens=p)
    a.update(kw)
    L = _capi.lib()
    head = (a["B"], a["Sq"], a["lens"], a["off"], a["bound"], a["lmax"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"], a["kbs"], a["krs"], a["vbs"],
            a["vrs"])
    tail = (a["scale"], a["causal"], a["dtype"], None)
    if kv8:
        return L.awq_attn_prefill_kvcache_kv8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], *head, a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"],
                                              *tail)
    return L.awq_attn_prefill_kvcache(a["q"], a["k"], a["v"], a["out"], *head, *tail)


def _paged(p, kv8=False, **kw):
    a = dict(PAGED_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, lens=p)
    a.update(kw)
    L = _capi.lib()
    head = (a["bt"], a["B"], a["Sq"], a["lens"], a["off"], a["bound"], a["pages"], a["ps"], a["pps"], a["trs"], a["H"], a["Hkv"], a["Dh"], a["qbs"],
            a["qrs"], a["kps"], a["krs"], a["vps"], a["vrs"])
    tail = (a["scale"], a["causal"], a["dtype"], None)
    if kv8:
        return L.awq_attn_prefill_paged_kv8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], *head, a["ksps"], a["ksrs"], a["vsps"], a["vsrs"],
                                            *tail)
    return L.awq_attn_prefill_paged(a["q"], a["k"], a["v"], a["out"], *head, *tail)


@pytest.mark.parametrize("kv8", [False, True], ids=["T", "kv8"])
def test_attn_prefill_kvcache_argument_validation_returns_codes_without_launch(kv8):
    buf, p = _p16()
    for bad in (dict(Dh=32), dict(Dh=96), dict(Dh=72), dict(Dh=256), dict(H=6, Hkv=4), dict(B=0), dict(Sq=0), dict(Sq=-3), dict(H=0), dict(Hkv=0),
                dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8), dict(kbs=-256), dict(vbs=-256), dict(bound=0), dict(bound=-1),
                dict(bound=4101), dict(off=-1), dict(B=2 ** 20, Sq=2 ** 20)):   # the last: more 64-row q tiles than a grid holds
        assert _dense(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # any seqlen_q passes the shape phase -- 33 is the first size the split pair refuses -- and reaches the alignment phase
    for Sq in (1, 32, 33, 129, 512, 4096, 100000):
        assert _dense(p, kv8, Sq=Sq, q=p + 2) == AWQ_ERR_ALIGN, Sq
        assert _dense(p, kv8, Sq=Sq, lens=p + 2) == AWQ_ERR_ALIGN, Sq           # .. and the tail: the lengths' alignment is its last check
    assert _dense(p, kv8, bound=4100, lens=p + 2) == AWQ_ERR_ALIGN               # the bound may equal the cache length
    assert _dense(p, kv8, causal=0, lens=p + 2) == AWQ_ERR_ALIGN and _dense(p, kv8, off=0, lens=p + 2) == AWQ_ERR_ALIGN
    assert _dense(p, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "lens") + (("ks", "vs") if kv8 else ()):
        assert _dense(p, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):
        assert _dense(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    if kv8:
        assert _dense(p, kv8, ks=p + 2) == AWQ_ERR_ALIGN and _dense(p, kv8, vs=p + 2) == AWQ_ERR_ALIGN
        assert _dense(p, kv8, ksrs=1) == AWQ_ERR_SHAPE and _dense(p, kv8, vsrs=1) == AWQ_ERR_SHAPE
        assert _dense(p, kv8, ksbs=-2) == AWQ_ERR_SHAPE and _dense(p, kv8, vsbs=-2) == AWQ_ERR_SHAPE
        for name, val in (("kbs", 4100 * 256 + 8), ("krs", 264), ("vbs", 4100 * 256 + 8), ("vrs", 264)):  # strides in codes: multiples of 16
            assert _dense(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 512 * 1024 + 4), ("qrs", 1028), ("kbs", 4100 * 256 + 4), ("krs", 260), ("vbs", 4100 * 256 + 4), ("vrs", 260)):
        assert _dense(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    # the order of the phases: null before dtype before shape before alignment
    assert _dense(p, kv8, q=None, dtype=2, Dh=96) == AWQ_ERR_NULL and _dense(p, kv8, dtype=2, Dh=96, k=p + 2) == AWQ_ERR_DTYPE
    assert _dense(p, kv8, Dh=96, k=p + 2) == AWQ_ERR_SHAPE and _dense(p, kv8, k=p + 2, off=-1) == AWQ_ERR_ALIGN


@pytest.mark.parametrize("kv8", [False, True], ids=["T", "kv8"])
def test_attn_prefill_paged_argument_validation_returns_codes_without_launch(kv8):
    buf, p = _p16()
    for bad in (dict(ps=0), dict(ps=32), dict(ps=63), dict(ps=96), dict(ps=320 - 1), dict(ps=-64), dict(pages=0), dict(pages=-1), dict(pps=0),
                dict(pps=-2), dict(trs=15), dict(trs=0), dict(bound=4097), dict(pps=15, trs=15), dict(bound=0), dict(off=-1), dict(Dh=96),
                dict(H=6, Hkv=4), dict(B=0), dict(Sq=0), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8), dict(kps=-256),
                dict(vps=-256), dict(B=2 ** 20, Sq=2 ** 20)):
        assert _paged(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    for Sq in (1, 32, 33, 129, 512, 4096, 100000):
        assert _paged(p, kv8, Sq=Sq, q=p + 2) == AWQ_ERR_ALIGN, Sq
        assert _paged(p, kv8, Sq=Sq, lens=p + 2) == AWQ_ERR_ALIGN, Sq
    for ok in (dict(ps=64, pps=64, trs=64), dict(trs=16), dict(ps=192, pps=22, trs=22), dict(pages=1)):
        assert _paged(p, kv8, lens=p + 2, **ok) == AWQ_ERR_ALIGN, ok
    assert _paged(p, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "bt", "lens") + (("ks", "vs") if kv8 else ()):
        assert _paged(p, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out", "bt"):
        assert _paged(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    if kv8:
        assert _paged(p, kv8, ks=p + 2) == AWQ_ERR_ALIGN and _paged(p, kv8, vs=p + 2) == AWQ_ERR_ALIGN
        assert _paged(p, kv8, ksrs=1) == AWQ_ERR_SHAPE and _paged(p, kv8, vsrs=1) == AWQ_ERR_SHAPE
        assert _paged(p, kv8, ksps=-2) == AWQ_ERR_SHAPE and _paged(p, kv8, vsps=-2) == AWQ_ERR_SHAPE
        for name, val in (("kps", 256 * 256 + 8), ("krs", 264), ("vps", 256 * 256 + 8), ("vrs", 264)):
            assert _paged(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 512 * 1024 + 4), ("qrs", 1028), ("kps", 256 * 256 + 4), ("krs", 260), ("vps", 256 * 256 + 4), ("vrs", 260)):
        assert _paged(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name


def test_the_split_pair_entries_keep_their_refusal():
    """awq_attn_kvcache* and the plan still refuse seqlen_q * G > 128: this feature changes no existing behaviour."""
    buf, p = _p16()
    L = _capi.lib()
    s, c = ctypes.c_int(), ctypes.c_int()
    assert L.awq_attn_kvcache_plan(1, 32, 8, 128, 33, 4096, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_kvcache(p, p, p, p, 2, 33, p, 1, 4096, 4100, 8, 2, 128, 33 * 1024, 1024, 4100 * 256, 256, 4100 * 256, 256, 0.1, 1, 0, None, 0,
                              None) == AWQ_ERR_SHAPE


def test_ops_refuse_cpu_tensors():
    q = torch.zeros(2, 40, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_prefill_kvcache(q, kc, kc, lens, 256)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_prefill_paged(q, pool, pool, bt, lens, 256)


# ------------------------------------------------------------------------------------------------------------------------
# the module and the shim route by seqlen * G
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for the engine: records which attention entry the module calls."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a, **kw):
            self.calls.append(name)
            x = a[0]
            if name.startswith("rope_kv_store"):
                return torch.zeros(x.shape[0], x.shape[1], 8, 64, dtype=x.dtype)
            return torch.zeros_like(x)
        return fn


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_routes_long_chunks_to_the_one_pass_entries(kv_dtype, paged, monkeypatch):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=2,
                                            kv_layout="natural", kv_dtype=kv_dtype)
    kw = dict(block_table=torch.zeros(2, 2, dtype=torch.int32), page_size=64) if paged else {}
    pos, freqs = torch.zeros(2, dtype=torch.int32), torch.zeros(128, 64)
    tail = ("_paged" if paged else "") + ("_kv8" if kv_dtype else "")
    new = "attn_prefill_" + ("paged" if paged else "kvcache") + ("_kv8" if kv_dtype else "")
    for S, want in ((1, "attn_kvcache" + tail), (32, "attn_kvcache" + tail), (33, new), (96, new)):   # G = 4: 32 tokens are 128 rows
        spy.calls.clear()
        out = m(torch.zeros(2, S, 768, dtype=torch.float16), pos, freqs, **kw)
        assert out.shape == (2, S, 512) and spy.calls[-1] == want and len(spy.calls) == 2, (S, spy.calls)


def test_flash_attn_with_kvcache_serves_a_prompt_chunk_and_still_refuses_a_block_table():
    from llm_awq_amd import flash_attn_compat as F

    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    lens = torch.tensor([50, 90], dtype=torch.int32)
    for Sq in (33, 200):   # Sq * G > 128: reaches the engine, which refuses CPU tensors -- no NotImplementedError, no torch fallback
        q = torch.zeros(2, Sq, 8, 128, dtype=torch.float16)
        for served in (dict(cache_seqlens=lens), dict(cache_seqlens=60)):
            with pytest.raises(RuntimeError, match="GPU") as e:
                F.flash_attn_with_kvcache(q, kc, kc, causal=True, **served)
            assert not isinstance(e.value, NotImplementedError) and "attn_prefill_kvcache" in str(e.value), served
    with pytest.raises(NotImplementedError, match="block_table"):
        F.flash_attn_with_kvcache(torch.zeros(2, 200, 8, 128, dtype=torch.float16), kc, kc, cache_seqlens=lens, causal=True,
                                  block_table=torch.zeros(2, 4, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# the needle batches are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_the_axes_of_the_issue():
    names = {s["name"] for s in C.CASES}
    assert len(names) == len(C.CASES) and len(C.PAGED_CASES) == 2 * len(C.CASES)
    assert (C.H, C.HKV, C.SQS, C.HISTORIES, C.BOUND, C.PAGE_SIZES) == (8, 2, (33, 65, 130), (0, 31, 63, 64, 127, 191), 384, (64, 128))
    assert all(Sq * (C.H // C.HKV) > 128 for Sq in C.SQS) and C.PAD_COLS > 0
    main = [s for s in C.CASES if s.get("causal", True) and "over" in s["lens"]]
    for Sq in C.SQS:
        mine = [s for s in main if s["Sq"] == Sq]
        assert {s["Dh"] for s in mine} == {64, 128} and {s["dtype"] for s in mine} == {torch.float16, torch.bfloat16}
        assert {s["offset"] for s in mine} == {Sq, 0}
        assert {s["mode"] for s in mine} == {"diag", "scatter", "edges", "negscale", "pair", "decoy"}
        for s in mine:
            assert s["lens"] == tuple(h + Sq for h in C.HISTORIES) + (None, "over") and s["bound"] == C.BOUND
    pb = C.PrefillBatch(next(s for s in main if s["Sq"] == 130 and s["offset"] == 130))
    assert pb.seqlens_k.tolist() == [0, 31, 63, 64, 127, 191, -1, C.BOUND + 1 - 130] and pb.total()[-2:] == [129, C.BOUND + 1]
    assert not pb.active(pb.lens[-1]) and torch.isnan(pb.k_cache[-1]).all() and not pb.target[-1].any()
    assert pb.active(129) and not pb.target[6, 0].any() and pb.target[6, 1:].any()      # the slot at -1: one negative-limit row, 129 keys
    short = [s for s in C.CASES if s["name"].startswith("short")]
    assert len(short) == 4 and all(s["offset"] == 0 and any(n is not None and n < s["Sq"] for n in s["lens"]) for s in short)
    pb = C.PrefillBatch(short[0])
    assert not pb.target[0, :45].any() and pb.target[0, 45:].any() and not pb.target[5].any() and pb.seqlens_k[5] == -1
    assert sum(not s.get("causal", True) for s in C.CASES) == 4
    pp = C.PagedPrefill(C.PAGED_CASES[0])
    assert pp.table_full.stride(0) == pp.pps + C.PAD_COLS and pp.table.stride(0) > pp.table.shape[1]


@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_dense_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    pb = C.PrefillBatch(spec)
    for b, n in enumerate(pb.lens):  # every cache row that holds no key is NaN
        held = n if pb.active(n) else 0
        assert not torch.isnan(pb.k_cache[b, :held]).any() and torch.isnan(pb.k_cache[b, held:]).all() and torch.isnan(pb.v_cache[b, held:]).all()
    out = C.dense(pb)
    assert torch.equal(bits(out), bits(pb.target)) and not torch.isnan(pb.q).any()
    for mutant in C.LEN_MUTANTS:
        if C.len_mutant_applies(pb, mutant):
            assert not torch.equal(bits(C.dense(pb, mutant)), bits(pb.target)), mutant


@pytest.mark.parametrize("spec", C.PAGED_CASES, ids=C.case_id)
def test_paged_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    pp = C.PagedPrefill(spec)  # (asserts the gather and the NaN of every row that holds no key)
    assert torch.equal(bits(C.paged(pp)), bits(pp.batch.target))
    for mutant in C.PAGE_MUTANTS:
        if C.page_mutant_applies(pp, mutant):
            assert not torch.equal(bits(C.paged(pp, mutant)), bits(pp.batch.target)), mutant


def test_every_mutant_is_seen_by_some_case_of_every_page_size_it_can_show_at():
    seen = {m: 0 for m in C.LEN_MUTANTS}
    for spec in C.CASES:
        if spec["dtype"] == torch.float16:
            pb = C.PrefillBatch(spec)
            for m in C.LEN_MUTANTS:
                seen[m] += C.len_mutant_applies(pb, m)
    assert all(v > 0 for v in seen.values()), seen
    for ps in C.PAGE_SIZES:
        seen = {m: 0 for m in C.PAGE_MUTANTS}
        for spec in C.PAGED_CASES:
            if spec["page_size"] == ps and spec["dtype"] == torch.float16:
                pp = C.PagedPrefill(spec)
                for m in C.PAGE_MUTANTS:
                    seen[m] += C.page_mutant_applies(pp, m)
        cannot = {"slot64"} if ps == 64 else set()   # a 64-row page has no row 64
        assert all(v > 0 for m, v in seen.items() if m not in cannot) and all(seen[m] == 0 for m in cannot), (ps, seen)
