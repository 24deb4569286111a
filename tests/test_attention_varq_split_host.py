"""A mixed packed step ("who serves a sequence"), without a GPU: the exports at every layer, the split plan and its workspace, every argument
check of the four C entries, of ops.attn_varq and of the module before any work, and the rule's restatement of
tests/attn_varq_split_cases.py with its mutants -- the step tests/test_gpu_attention_varq_split.py runs through the kernels tells each
mutant from the true rule by at least one sequence's route."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_varq_split_cases as S

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
ENTRIES = ("awq_attn_varq", "awq_attn_varq_kv8", "awq_attn_paged_varq", "awq_attn_paged_varq_kv8")
ONE_PASS = ("awq_attn_prefill_kvcache_varq", "awq_attn_prefill_kvcache_varq_kv8", "awq_attn_prefill_paged_varq", "awq_attn_prefill_paged_varq_kv8")
LL, I, VP, F, SZ = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------
def test_library_header_engine_and_ops_export_the_mixed_step():
    L = ctypes.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    for name in ENTRIES + ("awq_attn_varq_split_plan",):
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert hasattr(L, "awq_attn_varq_split_workspace_bytes") and re.search(r"\bsize_t awq_attn_varq_split_workspace_bytes\(", header)
    assert _capi.lib().awq_abi_version() == 1      # symbols were added, none changed
    S_ = _capi.SIGNATURES
    for new, old in zip(ENTRIES, ONE_PASS):        # the one-pass entry's arguments, then the two thresholds and the workspace, then the stream
        assert list(S_[new][1]) == list(S_[old][1])[:-1] + [I, I, VP, SZ, VP], new
    assert S_["awq_attn_varq_split_plan"][1] == [I] * 6 + [ctypes.POINTER(I)] * 2
    assert S_["awq_attn_varq_split_workspace_bytes"] == (SZ, [I] * 6)
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    tail = ["cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "split_seqlen_q", "split_min_keys", "lens_before_step", "softmax_scale",
            "causal", "out"]
    assert params(eng.attn_varq) == ["q", "k_cache", "v_cache"] + tail
    assert params(eng.attn_varq_kv8) == ["q", "k_cache", "v_cache", "k_scale", "v_scale"] + tail
    assert params(eng.attn_paged_varq) == ["q", "k_pool", "v_pool", "block_table"] + tail
    assert params(eng.attn_paged_varq_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table"] + tail
    assert params(eng.attn_varq_split_plan) == ["batch", "nheads", "nheads_kv", "head_dim", "split_seqlen_q", "max_seqlen_k"]
    sig = inspect.signature(ops.attn_varq)
    assert list(sig.parameters) == ["q", "k", "v", "cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "split_seqlen_q", "split_min_keys",
                                    "lens_before_step", "block_table", "softmax_scale", "causal", "k_scale", "v_scale", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["split_seqlen_q"] == 1 and d["split_min_keys"] is None and d["lens_before_step"] is True and d["causal"] is True
    # the default floor is the host-length plan's: attn_splitkv_plan never splits below it
    assert ops.ATTN_SPLIT_MIN_KEYS == 2048
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, ops.ATTN_SPLIT_MIN_KEYS - 1)[0] == 1 and ops.attn_splitkv_plan(1, 32, 8, 128, 1, ops.ATTN_SPLIT_MIN_KEYS)[0] > 1
    assert ops.attn_varq_split_plan(4, 32, 8, 128, 1, 32768) == tuple(eng.attn_varq_split_plan(4, 32, 8, 128, 1, 32768))


# ------------------------------------------------------------------------------------------------------------------------
# the plan and the workspace
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def force_chunk():
    had = os.environ.get("AWQ_TUNING")
    yield lambda c: _capi.tune(attn_splitkv_chunk=c)
    _capi.tune(attn_splitkv_chunk=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def test_split_plan_is_the_kvcache_plan_of_the_bound_and_honours_the_knob(force_chunk):
    L = _capi.lib()
    shapes = [(B, Hh, Hkv, Dh, q, bound) for B in (1, 10, 33) for (Hh, Hkv) in ((8, 2), (32, 8), (32, 32)) for Dh in (64, 128)
              for q in (0, 1, 4) for bound in (1, 512, 2048, 32768, 131072)]
    for forced in (0, 64, 256):
        force_chunk(forced)
        for B, Hh, Hkv, Dh, q, bound in shapes:
            splits, chunk = ops.attn_varq_split_plan(B, Hh, Hkv, Dh, q, bound)
            assert (splits, chunk) == ops.attn_kvcache_plan(B, Hh, Hkv, Dh, max(q, 1), bound), (forced, B, Hh, Hkv, Dh, q, bound)
            assert splits * chunk >= bound and chunk % 64 == 0 and (not forced or chunk == forced)
            assert L.awq_attn_varq_split_workspace_bytes(B, Hh, Hkv, Dh, q, bound) == B * Hh * q * splits * (Dh + 2) * 4
    force_chunk(64)
    assert ops.attn_varq_split_plan(10, 8, 2, 128, 8, 512) == (8, 64)           # the step of the GPU tests
    force_chunk(0)
    s, c = ctypes.c_int(), ctypes.c_int()
    assert L.awq_attn_varq_split_plan(1, 8, 2, 128, 1, 512, None, ctypes.byref(c)) == AWQ_ERR_NULL
    assert L.awq_attn_varq_split_plan(1, 8, 2, 128, 1, 512, ctypes.byref(s), None) == AWQ_ERR_NULL
    refused = [(1, 8, 2, 128, 33, 512),      # 33 * 4 rows per KV head
               (1, 32, 1, 128, 5, 512), (1, 8, 2, 72, 1, 512), (1, 8, 2, 96, 1, 512), (1, 8, 2, 128, -1, 512), (0, 8, 2, 128, 1, 512),
               (65536, 8, 2, 128, 1, 512), (1, 8, 3, 128, 1, 512), (1, 8, 2, 128, 1, 0)]
    for bad in refused:
        assert L.awq_attn_varq_split_plan(*bad, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE, bad
        assert L.awq_attn_varq_split_workspace_bytes(*bad) == 0, bad
        with pytest.raises(RuntimeError):
            ops.attn_varq_split_plan(*bad)
    assert L.awq_attn_varq_split_plan(1, 8, 2, 128, 32, 512, ctypes.byref(s), ctypes.byref(c)) == 0      # 32 * 4 = 128: the last that fits
    assert L.awq_attn_varq_split_plan(65535, 8, 2, 64, 0, 512, ctypes.byref(s), ctypes.byref(c)) == 0


# ------------------------------------------------------------------------------------------------------------------------
# argument validation of the four entries: every code, no GPU call.  A call that passed every check would launch: every call here is
# refused, and what passes a phase is shown by the code of a later one.
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


OK = dict(B=3, maxq=512, total=700, before=1, bound=4096, lmax=4100, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qrs=1024,
          kbs=4100 * 256, krs=256, vbs=4100 * 256, vrs=256, ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0,
          sq=1, floor=2048, wsb=1 << 40)


def _call(p, paged, kv8, **kw):
    a = dict(OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, cu=p, lens=p, ws=p)
    if paged:
        a.update(kbs=256 * 256, vbs=256 * 256, ksbs=512, vsbs=512)
    a.update(kw)
    step = (a["B"], a["cu"], a["maxq"], a["total"], a["lens"], a["before"], a["bound"])
    where = (a["bt"], *step, a["pages"], a["ps"], a["pps"], a["trs"]) if paged else (*step, a["lmax"])
    strides = (a["qrs"], a["kbs"], a["krs"], a["vbs"], a["vrs"]) + ((a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"]) if kv8 else ())
    fn = getattr(_capi.lib(), "awq_attn_" + ("paged_" if paged else "") + "varq" + ("_kv8" if kv8 else ""))
    return fn(a["q"], a["k"], a["v"], *((a["ks"], a["vs"]) if kv8 else ()), a["out"], *where, a["H"], a["Hkv"], a["Dh"], *strides, a["scale"],
              a["causal"], a["dtype"], a["sq"], a["floor"], a["ws"], a["wsb"], None)


FORMS = [(False, False), (False, True), (True, False), (True, True)]
FORM_IDS = ["dense-T", "dense-fp8", "paged-T", "paged-fp8"]


@pytest.mark.parametrize("paged,kv8", FORMS, ids=FORM_IDS)
def test_entries_return_every_code_without_a_launch(paged, kv8):
    buf, p = _p16()
    L = _capi.lib()
    need = L.awq_attn_varq_split_workspace_bytes(3, 8, 2, 128, 1, 4096)
    assert need == 3 * 8 * 1 * ops.attn_varq_split_plan(3, 8, 2, 128, 1, 4096)[0] * 130 * 4 > 0
    # the split terms of the shape phase
    for bad in (dict(sq=-1), dict(sq=-7), dict(floor=0), dict(floor=-3), dict(sq=33), dict(sq=2, H=128, Hkv=1), dict(sq=0, floor=0)):
        assert _call(p, paged, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # the one-pass entries' shape terms stay
    bad_shapes = [dict(maxq=0), dict(total=0), dict(B=0), dict(B=65536), dict(Dh=96), dict(Dh=72), dict(H=6, Hkv=4), dict(H=0), dict(Hkv=0),
                  dict(qrs=512), dict(krs=128), dict(bound=0)]
    bad_shapes += [dict(ps=96), dict(pages=0), dict(pps=0), dict(trs=15), dict(bound=4097)] if paged else [dict(bound=4101)]
    for bad in bad_shapes:
        assert _call(p, paged, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # what passes the shape phase reaches the alignment phase and, behind the lengths' alignment, the workspace
    for ok in (dict(sq=1), dict(sq=32), dict(sq=0), dict(floor=1), dict(floor=2 ** 31 - 1), dict(maxq=1), dict(before=0), dict(causal=0)):
        assert _call(p, paged, kv8, cu=p + 2, **ok) == AWQ_ERR_ALIGN, ok
        assert _call(p, paged, kv8, lens=p + 2, **ok) == AWQ_ERR_ALIGN, ok
        if ok.get("sq", 1) > 0:
            assert _call(p, paged, kv8, ws=None, **ok) == AWQ_ERR_WORKSPACE, ok
            assert _call(p, paged, kv8, wsb=0, **ok) == AWQ_ERR_WORKSPACE, ok
    assert _call(p, paged, kv8, wsb=need - 1) == AWQ_ERR_WORKSPACE        # one byte short
    assert _call(p, paged, kv8, wsb=need, ws=p + 4) == AWQ_ERR_ALIGN      # enough bytes: the workspace's own alignment is the last check
    assert _call(p, paged, kv8, wsb=need - 1, ws=p + 4) == AWQ_ERR_WORKSPACE
    assert _call(p, paged, kv8, sq=8, wsb=8 * need - 1) == AWQ_ERR_WORKSPACE and _call(p, paged, kv8, sq=8, wsb=8 * need, ws=p + 8) == AWQ_ERR_ALIGN
    assert _call(p, paged, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "cu", "lens") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
        assert _call(p, paged, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out", "cu") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
        assert _call(p, paged, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    # the order of the phases: null before dtype before shape before alignment before the workspace
    assert _call(p, paged, kv8, cu=None, dtype=2, sq=-1) == AWQ_ERR_NULL and _call(p, paged, kv8, dtype=2, sq=-1, ws=None) == AWQ_ERR_DTYPE
    assert _call(p, paged, kv8, floor=0, cu=p + 2, ws=None) == AWQ_ERR_SHAPE and _call(p, paged, kv8, cu=p + 2, ws=None) == AWQ_ERR_ALIGN


def test_ops_attn_varq_raises_before_any_work():
    q = torch.zeros(40, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    # the two thresholds are checked first: CPU tensors never get as far as the GPU check
    for kw, text in ((dict(split_seqlen_q=-1), "split_seqlen_q -1 must not be negative"), (dict(split_min_keys=0), "split_min_keys 0 must be at least 1"),
                     (dict(split_min_keys=-5), "at least 1"), (dict(split_seqlen_q=-2, split_min_keys=0), "split_seqlen_q")):
        for extra in (dict(), dict(block_table=bt)):
            with pytest.raises(ValueError, match=text):
                ops.attn_varq(q, pool if extra else kc, pool if extra else kc, cu, 30, lens, 256, **kw, **extra)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_varq(q, kc, kc, cu, 30, lens, 256)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_varq(q, pool, pool, cu, 30, lens, 256, split_seqlen_q=0, block_table=bt)


# ------------------------------------------------------------------------------------------------------------------------
# the module: forward_packed is today's path, forward_packed_split routes the attention to the mixed entries
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for the engine: records the entry and the arguments of every call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a, **kw):
            self.calls.append((name, a, kw))
            x = a[0]
            if name.startswith("rope_kv_store"):
                return torch.zeros(*x.shape[:-1], 8, 64, dtype=x.dtype)
            return torch.zeros_like(x)
        return fn


def _module(monkeypatch, kv_dtype=None):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3,
                                            kv_layout="natural", kv_dtype=kv_dtype)
    return m, spy


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_routes_a_mixed_step_to_one_store_and_the_mixed_attention(kv_dtype, paged, monkeypatch):
    m, spy = _module(monkeypatch, kv_dtype)
    table = torch.zeros(3, 2, dtype=torch.int32)
    kw = dict(block_table=table, page_size=64) if paged else {}
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    out = m.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=2, split_min_keys=64, **kw)
    assert out.shape == (1, 140, 512) and len(spy.calls) == 2
    (store, sa, _), (attn, aa, _) = spy.calls
    assert store == "rope_kv_store_" + ("paged" if paged else "natural") + "_varq" + ("_fp8" if kv_dtype else "")
    assert attn == "attn" + ("_paged" if paged else "") + "_varq" + ("_kv8" if kv_dtype else "")
    nkv = 4 if kv_dtype else 2
    i = 1 + nkv + paged
    assert aa[0].shape == (140, 8, 64) and len(aa) == i + 9
    assert aa[i] is cu and aa[i + 1] == 96 and aa[i + 2] is pos and aa[i + 3] == 128
    assert aa[i + 4:i + 7] == (2, 64, True) and aa[-1] is True             # the two thresholds, lens_before_step; causal
    spy.calls.clear()
    m.forward_packed_split(x, pos, freqs, cu, 96, **kw)                    # the defaults: one new token, the plan's floor
    assert spy.calls[1][1][i + 4:i + 6] == (1, ops.ATTN_SPLIT_MIN_KEYS)
    # forward_packed itself is unchanged: its parameter list, its two entries and their arguments
    spy.calls.clear()
    m.forward_packed(x, pos, freqs, cu, 96, **kw)
    assert [c[0] for c in spy.calls] == [store, "attn_prefill" + ("_paged" if paged else "") + "_varq" + ("_kv8" if kv_dtype else "")]
    assert len(spy.calls[1][1]) == i + 7 and spy.calls[1][1][i + 4] is True
    assert list(inspect.signature(m.forward_packed).parameters) == ["x", "start_pos", "freqs", "cu_seqlens_q", "max_seqlen_q", "decode_max_seqlen",
                                                                    "block_table", "page_size"]
    assert list(inspect.signature(m.forward_packed_split).parameters) == ["x", "start_pos", "freqs", "cu_seqlens_q", "max_seqlen_q", "split_seqlen_q",
                                                                          "split_min_keys", "decode_max_seqlen", "block_table", "page_size"]


def test_module_refuses_bad_thresholds_before_any_work(monkeypatch):
    m, spy = _module(monkeypatch)
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    for kw, text in ((dict(split_seqlen_q=-1), "split_seqlen_q -1 must lie in 0 .. 32"), (dict(split_seqlen_q=33), "split_seqlen_q 33"),
                     (dict(split_min_keys=0), "split_min_keys 0 must be at least 1"), (dict(split_seqlen_q=1, split_min_keys=-1), "at least 1")):
        with pytest.raises(ValueError, match=text):
            m.forward_packed_split(x, pos, freqs, cu, 96, **kw)
    with pytest.raises(ValueError, match="come together"):                 # forward_packed's own checks stand in front of the work too
        m.forward_packed_split(x, pos, freqs, None, 96)
    with pytest.raises(ValueError, match="at least 1"):
        m.forward_packed_split(x, pos, freqs, cu, 0)
    assert not spy.calls


# ------------------------------------------------------------------------------------------------------------------------
# the rule on the CPU: the step decides every term, and every mutant changes some sequence's route
# ------------------------------------------------------------------------------------------------------------------------
def test_step_is_the_one_the_gpu_tests_run():
    assert (S.H, S.HKV, S.BOUND, S.LMAX, S.CHUNK, S.SPLIT_MIN_KEYS, S.SPLIT_SEQLEN_Q, S.MAX_Q, S.PAD_ROWS) == (8, 2, 512, 519, 64, 128, 8, 70, 9)
    assert S.STEP == ((1, 256), (1, 127), (1, 126), (8, 200), (9, 300), (0, 500), (70, 64), (1, -1), (3, 509), (2, 511))
    assert S.SPLIT_SEQLEN_Q * S.G <= 128 and S.PAGE_SIZES == (64, 128) and S.COMBOS == [
        (torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)]
    assert S.routes(True) == S.TAKEN == S.routes(False)
    assert [S.active(b) for b in range(10)] == [True] * 7 + [False, True, False]
    st = S.Step(torch.float16, 64)
    assert st.cu == [0, 1, 2, 3, 11, 20, 20, 90, 91, 94, 96] and st.total_q == 105 and st.held == [257, 128, 127, 208, 309, 500, 134, 0, 512, 0]
    assert torch.isnan(st.q[96:]).all() and not torch.isnan(st.q[:96]).any()
    for b, n in enumerate(st.held):     # NaN in every cache row that holds no key
        assert not torch.isnan(st.k_cache[b, :n]).any() and torch.isnan(st.k_cache[b, n:]).all() and torch.isnan(st.v_cache[b, n:]).all()
    assert st.seqlens_k(True).tolist() == [h for _, h in S.STEP] and st.seqlens_k(False).tolist() == [h + n for n, h in S.STEP]
    for ps in S.PAGE_SIZES:
        pool = S.Pool(st, ps)
        assert pool.table_full.stride(0) == pool.pps + S.PAD_COLS and pool.pps * ps == S.BOUND
        for b, n in enumerate(st.held):
            k, v = pool.gather(b, n)
            assert torch.equal(k.view(torch.int16), st.k_cache[b, :n].view(torch.int16)) and torch.equal(v.view(torch.int16), st.v_cache[b, :n].view(torch.int16))
            assert (pool.table[b, (n + ps - 1) // ps:] == pool.poison).all()
        used = set(pool.table_full.flatten().tolist()) - {pool.poison}
        held = sum((n + ps - 1) // ps for n in st.held)
        assert len(used) == held and torch.isnan(pool.k_pool[pool.poison]).all() and torch.isnan(pool.v_pool[pool.poison]).all()


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_the_step_tells_every_mutant_from_the_rule(mutant):
    true, wrong = S.routes(True), S.routes(True, mutant)
    diff = [b for b in range(len(S.STEP)) if true[b] != wrong[b]]
    assert diff, mutant
    want = {"floor+1": [1], "floor-1": [2], "sq+1": [4], "sq-1": [3], "before-off": [1, 9], "inactive-taken": [9]}[mutant]   # (before-off: 511 keys are inside the bound)
    assert diff == want, (mutant, diff)
    if mutant != "before-off":          # with total lengths the flag has nothing to ignore; every other mutant is seen there too
        assert S.routes(False) != S.routes(False, mutant), mutant


def test_rule_edges():
    t = S.takes
    assert t(1, 127, True) and not t(1, 126, True) and t(1, 128, False) and not t(1, 127, False)
    assert t(8, 120, True) and not t(9, 300, True) and not t(0, 500, True) and not t(1, -1, True)
    assert t(3, 509, True) and not t(2, 511, True) and not t(1, 512, True) and t(1, 511, True)
    assert not t(1, 300, True, split_q=0)                                   # split_seqlen_q = 0: nothing is taken
    assert not t(5, 300, True, max_q=4, split_q=8) and t(4, 300, True, max_q=4, split_q=8)    # beyond max_seqlen_q: inactive, not taken
    assert t(1, 2 ** 31 - 2, True, bound=2 ** 31 - 1) and not t(1, 2 ** 31 - 1, True, bound=2 ** 31 - 1)   # formed beyond 32 bits
