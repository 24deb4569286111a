"""Per-sequence query lengths on the KV-cache path ("varq"), without a GPU: the nine exports at every layer, every argument check of the C
ABI, the plan's rule, the module's and the shim's routing, and the soundness of the packed batches of tests/attn_varq_cases.py -- the
lists tests/test_gpu_attention_varq.py runs through the kernels -- against the float64 restatement of the calls and each of its mutants."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_varq_cases as V

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL = -3, -4, -5, -6
ATTN = ("awq_attn_prefill_kvcache_varq", "awq_attn_prefill_kvcache_varq_kv8", "awq_attn_prefill_paged_varq", "awq_attn_prefill_paged_varq_kv8")
STORE = ("awq_rope_kv_store_natural_varq", "awq_rope_kv_store_natural_varq_fp8", "awq_rope_kv_store_paged_varq", "awq_rope_kv_store_paged_varq_fp8")
LL, I, VP, F = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------
def test_library_header_engine_and_ops_export_the_varq_surface():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    for name in ATTN + STORE + ("awq_attn_varq_plan",):
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    packed = ["cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "lens_before_step", "softmax_scale", "causal", "out"]
    assert params(eng.attn_prefill_varq) == ["q", "k_cache", "v_cache"] + packed
    assert params(eng.attn_prefill_varq_kv8) == ["q", "k_cache", "v_cache", "k_scale", "v_scale"] + packed
    assert params(eng.attn_prefill_paged_varq) == ["q", "k_pool", "v_pool", "block_table"] + packed
    assert params(eng.attn_prefill_paged_varq_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table"] + packed
    tail = ["cu_seqlens_q", "max_seqlen_q", "cache_seqlens", "nheads", "nheads_kv", "q_out"]
    assert params(eng.rope_kv_store_natural_varq) == ["qkv", "freqs_table", "k_cache", "v_cache"] + tail
    assert params(eng.rope_kv_store_natural_varq_fp8) == ["qkv", "freqs_table", "k_cache", "v_cache", "k_scale", "v_scale"] + tail
    assert params(eng.rope_kv_store_paged_varq) == ["qkv", "freqs_table", "k_pool", "v_pool", "block_table"] + tail
    assert params(eng.rope_kv_store_paged_varq_fp8) == ["qkv", "freqs_table", "k_pool", "v_pool", "k_scale", "v_scale", "block_table"] + tail
    assert params(eng.attn_varq_plan) == ["batch", "nheads", "nheads_kv", "head_dim", "max_seqlen_q"]
    assert list(inspect.signature(ops.rope_kv_store_varq).parameters)[:12] == [
        "qkv", "freqs_table", "k", "v", "cu_seqlens_q", "max_seqlen_q", "cache_seqlens", "nheads", "nheads_kv", "block_table", "k_scale", "v_scale"]
    sig = inspect.signature(ops.attn_prefill_varq)
    assert list(sig.parameters)[:13] == ["q", "k", "v", "cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "lens_before_step",
                                         "block_table", "softmax_scale", "causal", "k_scale", "v_scale"]
    assert sig.parameters["lens_before_step"].default is True and sig.parameters["causal"].default is True
    assert ops.attn_varq_plan(4, 32, 8, 128, 512) == tuple(eng.attn_varq_plan(4, 32, 8, 128, 512))


def test_capi_signatures_are_the_rectangular_entries_with_the_packed_step():
    S = _capi.SIGNATURES
    for new, old in zip(ATTN, ("awq_attn_prefill_kvcache", "awq_attn_prefill_kvcache_kv8", "awq_attn_prefill_paged", "awq_attn_prefill_paged_kv8")):
        args, oargs = list(S[new][1]), list(S[old][1])
        i = oargs.index(I)                                    # batch; seqlen_q follows it
        assert oargs[i:i + 3] == [I, I, VP] and args[:i] == oargs[:i] and args[i:i + 5] == [I, VP, I, I, VP], new
        rest, orest = args[i + 5:], oargs[i + 3:]
        # one long long fewer: q has no batch stride
        assert len(rest) == len(orest) - 1 and rest.count(LL) == orest.count(LL) - 1 and rest[-4:] == [F, I, I, VP], new
    for new, old in zip(STORE, ("awq_rope_kv_store_natural_pos", "awq_rope_kv_store_natural_pos_fp8", "awq_rope_kv_store_paged_pos",
                                "awq_rope_kv_store_paged_pos_fp8")):
        args, oargs = list(S[new][1]), list(S[old][1])
        # (batch .., seqlen) -> (batch .., cu_seqlens_q, max_seqlen_q, total_q): one pointer and one int more, one long long fewer
        assert args.count(VP) == oargs.count(VP) + 1 and args.count(I) == oargs.count(I) + 1 and args.count(LL) == oargs.count(LL) - 1, new
    assert S["awq_attn_prefill_kvcache_varq"][1] == [VP] * 4 + [I, VP, I, I, VP] + [I] * 6 + [LL] * 5 + [F, I, I, VP]
    assert S["awq_rope_kv_store_paged_varq_fp8"][1] == [VP] * 9 + [I, VP] + [I] * 10 + [LL] * 10 + [I, VP]
    assert S["awq_attn_varq_plan"][1] == [I] * 5 + [ctypes.POINTER(I)] * 2


# ------------------------------------------------------------------------------------------------------------------------
# the plan: 64 rows while max_seqlen_q <= 64, else attn_prefill_plan's choice for max_seqlen_q capped at 128 (a provisional rule)
# ------------------------------------------------------------------------------------------------------------------------
def test_varq_plan_rule():
    for B, Hh, Hkv in ((1, 8, 2), (4, 32, 8), (64, 32, 8), (512, 32, 8)):
        for Dh in (64, 128):
            for M in (1, 17, 64, 65, 128, 129, 130, 512, 1024, 4096):
                rows, blocks = ops.attn_varq_plan(B, Hh, Hkv, Dh, M)
                want = 64 if M <= 64 else min(128, ops.attn_prefill_plan(B, Hh, Hkv, Dh, M, M)[0])
                assert rows == want and rows in (64, 128) and blocks == B * Hh * ((M + rows - 1) // rows), (B, Hh, Dh, M, rows, blocks)
    assert ops.attn_prefill_plan(64, 32, 8, 128, 4096, 4096)[0] == 256 and ops.attn_varq_plan(64, 32, 8, 128, 4096)[0] == 128  # the cap
    try:
        for forced, want in ((64, 64), (128, 128), (256, 128), (0, 128)):   # a forced 256 leaves the plan's own choice in place
            _capi.tune(attn_prefill_rows=forced)
            assert ops.attn_varq_plan(64, 32, 8, 128, 4096)[0] == want, forced
        _capi.tune(attn_prefill_rows=128)
        assert ops.attn_varq_plan(1, 8, 2, 64, 17)[0] == 128
        _capi.tune(attn_prefill_rows=256)
        assert ops.attn_varq_plan(1, 8, 2, 64, 17)[0] == 64
    finally:
        _capi.tune(attn_prefill_rows=0)
    r, b = ctypes.c_int(), ctypes.c_int()
    L = _capi.lib()
    assert L.awq_attn_varq_plan(1, 8, 2, 128, 64, None, ctypes.byref(b)) == AWQ_ERR_NULL
    for bad in ((0, 8, 2, 128, 64), (1, 8, 3, 128, 64), (1, 8, 2, 96, 64), (1, 8, 2, 128, 0), (65536, 8, 2, 128, 64), (65535, 2 ** 15, 1, 128, 2 ** 20)):
        assert L.awq_attn_varq_plan(*bad, ctypes.byref(r), ctypes.byref(b)) == AWQ_ERR_SHAPE, bad
    assert L.awq_attn_varq_plan(65535, 8, 2, 128, 64, ctypes.byref(r), ctypes.byref(b)) == 0


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call.  A call that passed every check would launch: every call here is refused, and a shape is
# shown to PASS the shape phase by the code of a later phase (alignment).
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


ATTN_OK = dict(B=3, maxq=512, total=700, before=1, bound=4096, lmax=4100, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qrs=1024,
               kbs=4100 * 256, krs=256, vbs=4100 * 256, vrs=256, ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0)
STORE_OK = dict(B=3, cb=4, maxq=512, total=700, H=8, Hkv=2, Dh=128, rot=128, lmax=4100, P=8192, pages=40, ps=256, pps=16, trs=20, kps=256 * 256,
                krs=256, vps=256 * 256, vrs=256, ksps=512, ksrs=2, vsps=512, vsrs=2, rs=1536, dtype=0)


def _attn(p, paged, kv8, **kw):
    a = dict(ATTN_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, cu=p, lens=p)
    if paged:
        a.update(kbs=256 * 256, vbs=256 * 256, ksbs=512, vsbs=512)
    a.update(kw)
    step = (a["B"], a["cu"], a["maxq"], a["total"], a["lens"], a["before"], a["bound"])
    where = (a["bt"], *step, a["pages"], a["ps"], a["pps"], a["trs"]) if paged else (*step, a["lmax"])
    strides = (a["qrs"], a["kbs"], a["krs"], a["vbs"], a["vrs"]) + ((a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"]) if kv8 else ())
    fn = getattr(_capi.lib(), "awq_attn_prefill_" + ("paged" if paged else "kvcache") + "_varq" + ("_kv8" if kv8 else ""))
    return fn(a["q"], a["k"], a["v"], *((a["ks"], a["vs"]) if kv8 else ()), a["out"], *where, a["H"], a["Hkv"], a["Dh"], *strides, a["scale"],
              a["causal"], a["dtype"], None)


def _store(p, paged, fp8, **kw):
    a = dict(STORE_OK, qkv=p, fr=p, qo=p, k=p, v=p, ks=p, vs=p, bt=p, pos=p, cu=p)
    a.update(kw)
    head = (a["qkv"], a["fr"], a["qo"], a["k"], a["v"]) + ((a["ks"], a["vs"]) if fp8 else ())
    step = (a["cu"], a["maxq"], a["total"], a["H"], a["Hkv"], a["Dh"], a["rot"])
    fn = getattr(_capi.lib(), "awq_rope_kv_store_" + ("paged" if paged else "natural") + "_varq" + ("_fp8" if fp8 else ""))
    if paged:
        strides = (a["trs"], a["kps"], a["krs"], a["vps"], a["vrs"]) + ((a["ksps"], a["ksrs"], a["vsps"], a["vsrs"]) if fp8 else ())
        return fn(*head, a["bt"], a["pos"], a["B"], *step, a["P"], a["pages"], a["ps"], a["pps"], *strides, a["rs"], a["dtype"], None)
    return fn(*head, a["pos"], a["B"], a["cb"], *step, a["lmax"], a["P"], a["rs"], a["dtype"], None)


FORMS = [(False, False), (False, True), (True, False), (True, True)]
FORM_IDS = ["dense-T", "dense-fp8", "paged-T", "paged-fp8"]


@pytest.mark.parametrize("paged,kv8", FORMS, ids=FORM_IDS)
def test_attention_entries_return_every_code_without_a_launch(paged, kv8):
    buf, p = _p16()
    bad_shapes = [dict(maxq=0), dict(maxq=-1), dict(total=0), dict(total=-5), dict(B=0), dict(B=65536), dict(B=65535, H=2 ** 15, Hkv=1, maxq=2 ** 20),
                  dict(Dh=96), dict(Dh=72), dict(H=6, Hkv=4), dict(H=0), dict(Hkv=0), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(kbs=-256),
                  dict(vbs=-256), dict(bound=0), dict(bound=-1)]
    bad_shapes += [dict(ps=0), dict(ps=96), dict(pages=0), dict(pps=0), dict(trs=15), dict(bound=4097)] if paged else [dict(bound=4101)]
    for bad in bad_shapes:
        assert _attn(p, paged, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # what passes the shape phase reaches the alignment phase: any max_seqlen_q, either flag value, total_q below or above the bound
    for ok in (dict(maxq=1), dict(maxq=64), dict(maxq=65), dict(maxq=100000), dict(before=0), dict(before=7), dict(total=1), dict(total=2 ** 30),
               dict(B=65535), dict(causal=0)):
        assert _attn(p, paged, kv8, cu=p + 2, **ok) == AWQ_ERR_ALIGN, ok
        assert _attn(p, paged, kv8, lens=p + 2, **ok) == AWQ_ERR_ALIGN, ok      # the tail: the lengths' alignment is the last check
    assert _attn(p, paged, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "cu", "lens") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
        assert _attn(p, paged, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out", "cu") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
        assert _attn(p, paged, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _attn(p, paged, kv8, cu=p + 4, lens=p + 2) == AWQ_ERR_ALIGN and _attn(p, paged, kv8, cu=p + 1) == AWQ_ERR_ALIGN
    for name, val in (("qrs", 1028), ("krs", 260), ("vrs", 260)):
        assert _attn(p, paged, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    # the order of the phases: null before dtype before shape before alignment
    assert _attn(p, paged, kv8, cu=None, dtype=2, maxq=0) == AWQ_ERR_NULL and _attn(p, paged, kv8, dtype=2, maxq=0, cu=p + 2) == AWQ_ERR_DTYPE
    assert _attn(p, paged, kv8, maxq=0, cu=p + 2) == AWQ_ERR_SHAPE and _attn(p, paged, kv8, total=0, q=p + 2) == AWQ_ERR_SHAPE


@pytest.mark.parametrize("paged,fp8", FORMS, ids=FORM_IDS)
def test_store_entries_return_every_code_without_a_launch(paged, fp8):
    buf, p = _p16()
    bad_shapes = [dict(maxq=0), dict(maxq=-1), dict(total=0), dict(total=-5), dict(B=0), dict(B=65536)]
    bad_shapes += [dict(Dh=96), dict(H=0), dict(Hkv=0), dict(rot=8), dict(rot=24), dict(rot=256), dict(rs=1535), dict(rs=1024), dict(P=0)]
    bad_shapes += [dict(ps=0), dict(ps=96), dict(pages=0), dict(pps=0), dict(trs=15), dict(krs=128), dict(vrs=128)] if paged else \
                  [dict(cb=2), dict(lmax=0)]
    for bad in bad_shapes:
        assert _store(p, paged, fp8, **bad) == AWQ_ERR_SHAPE, bad
    for ok in (dict(maxq=1), dict(maxq=100000), dict(total=1), dict(total=2 ** 30), dict(B=65535, cb=65535)):
        assert _store(p, paged, fp8, cu=p + 2, **ok) == AWQ_ERR_ALIGN, ok
    assert _store(p, paged, fp8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "fr", "qo", "k", "v", "pos", "cu") + (("ks", "vs") if fp8 else ()) + (("bt",) if paged else ()):
        assert _store(p, paged, fp8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("qkv", "fr", "qo", "k", "v", "pos", "cu") + (("ks", "vs") if fp8 else ()) + (("bt",) if paged else ()):
        assert _store(p, paged, fp8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _store(p, paged, fp8, rs=1540) == AWQ_ERR_ALIGN
    assert _store(p, paged, fp8, cu=None, dtype=2, maxq=0) == AWQ_ERR_NULL and _store(p, paged, fp8, dtype=2, maxq=0, cu=p + 2) == AWQ_ERR_DTYPE
    assert _store(p, paged, fp8, maxq=0, cu=p + 2) == AWQ_ERR_SHAPE


def test_ops_refuse_cpu_tensors():
    q = torch.zeros(40, 8, 128, dtype=torch.float16)
    qkv = torch.zeros(40, 12 * 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    fr = torch.zeros(512, 128)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_prefill_varq(q, kc, kc, cu, 30, lens, 256)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_prefill_varq(q, pool, pool, cu, 30, lens, 256, block_table=bt)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.rope_kv_store_varq(qkv, fr, kc, kc, cu, 30, lens, 8, 2)


# ------------------------------------------------------------------------------------------------------------------------
# the module and the shim route a packed step to the varq entries
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


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_routes_a_packed_step_to_one_store_and_one_attention(kv_dtype, paged, monkeypatch):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3,
                                            kv_layout="natural", kv_dtype=kv_dtype)
    table = torch.zeros(3, 2, dtype=torch.int32)
    kw = dict(block_table=table, page_size=64) if paged else {}
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    out = m.forward_packed(x, pos, freqs, cu, 96, **kw)
    assert out.shape == (1, 140, 512) and len(spy.calls) == 2
    (store, sa, _), (attn, aa, _) = spy.calls
    assert store == "rope_kv_store_" + ("paged" if paged else "natural") + "_varq" + ("_fp8" if kv_dtype else "")
    assert attn == "attn_prefill" + ("_paged" if paged else "") + "_varq" + ("_kv8" if kv_dtype else "")
    nkv = 4 if kv_dtype else 2
    assert sa[0].shape == (140, 768) and sa[1] is freqs and sa[-5] is cu and sa[-4] == 96 and sa[-3] is pos and sa[-2:] == (8, 2)
    assert aa[0].shape == (140, 8, 64) and len(aa) == 1 + nkv + paged + 7
    assert aa[1 + nkv + paged] is cu and aa[2 + nkv + paged] == 96 and aa[3 + nkv + paged] is pos
    assert aa[4 + nkv + paged] == 128 and aa[5 + nkv + paged] is True and aa[-1] is True          # the bound, lens_before_step, causal
    if paged:
        assert sa[2 + nkv] is table and aa[1 + nkv] is table and sa[2].shape == (6, 64, 2, 64)
    # forward itself is unchanged: its parameter list, and the rectangular route
    assert list(inspect.signature(m.forward).parameters)[-2:] == ["block_table", "page_size"]
    assert list(inspect.signature(m.forward_packed).parameters) == ["x", "start_pos", "freqs", "cu_seqlens_q", "max_seqlen_q", "decode_max_seqlen",
                                                                    "block_table", "page_size"]
    spy.calls.clear()
    m(torch.zeros(3, 40, 768, dtype=torch.float16), pos, freqs, **kw)
    assert [c[0] for c in spy.calls] == ["rope_kv_store_" + ("paged_pos" if paged else "natural_pos") + ("_fp8" if kv_dtype else ""),
                                         "attn_prefill_" + ("paged" if paged else "kvcache") + ("_kv8" if kv_dtype else "")]


def test_module_refuses_a_malformed_packed_call_before_any_work(monkeypatch):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3, kv_layout="natural")
    ft = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3)
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    for mod, xx, pp, kw, text in ((m, x, pos, dict(cu_seqlens_q=cu), "come together"), (m, x, pos, dict(max_seqlen_q=96), "come together"),
                                  (ft, x, pos, dict(cu_seqlens_q=cu, max_seqlen_q=96), "kv_layout 'natural'"),
                                  (m, x, 0, dict(cu_seqlens_q=cu, max_seqlen_q=96), "int32 tensor \\[B\\]"),
                                  (m, x, pos, dict(cu_seqlens_q=cu[:3], max_seqlen_q=96), "\\[B \\+ 1\\]"),
                                  (m, x, pos, dict(cu_seqlens_q=cu.long(), max_seqlen_q=96), "\\[B \\+ 1\\]"),
                                  (m, x.view(2, 70, 768), pos, dict(cu_seqlens_q=cu, max_seqlen_q=96), "\\[1, T, hidden\\]"),
                                  (m, x, pos, dict(cu_seqlens_q=cu, max_seqlen_q=0), "at least 1")):
        with pytest.raises(ValueError, match=text):
            mod.forward_packed(xx, pp, freqs, **dict(dict(cu_seqlens_q=None, max_seqlen_q=None), **kw))
    with pytest.raises(ValueError, match="come together"):
        m.forward_packed(x, pos, freqs, cu, 96, block_table=torch.zeros(3, 2, dtype=torch.int32))      # the paged pair's own check
    assert not spy.calls


def test_flash_attn_varlen_func_routes_to_the_paged_varq_entry(monkeypatch):
    import llm_awq_amd
    from llm_awq_amd import flash_attn_compat as F

    assert F.flash_attn_interface.flash_attn_varlen_func is F.flash_attn_varlen_func and "flash_attn_varlen_func" in F.__all__
    spy = _Spy()
    monkeypatch.setattr(llm_awq_amd, "load_engine", lambda: spy)
    q = torch.zeros(50, 8, 128, dtype=torch.float16)
    pool = torch.zeros(6, 64, 2, 128, dtype=torch.float16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    cu_q = torch.tensor([0, 10, 50], dtype=torch.int32)
    cu_k = torch.tensor([0, 100, 150], dtype=torch.int32)
    out = F.flash_attn_varlen_func(q, pool, pool, cu_q, cu_k, 40, 192, causal=True, block_table=table)
    (name, a, _), = spy.calls
    assert out.shape == q.shape and name == "attn_prefill_paged_varq"
    assert a[0] is q and a[1] is pool and a[3] is table and a[4] is cu_q and a[5] == 40 and a[6].tolist() == [100, 50] and a[6].dtype == torch.int32
    assert a[7] == 192 and a[8] is False and a[9] == 128 ** -0.5 and a[10] is True     # total lengths: lens_before_step clear
    F.flash_attn_varlen_func(q, pool, pool, cu_q, cu_k, 40, 192, softmax_scale=0.5, block_table=table, deterministic=True, window_size=(-1, -1))
    assert spy.calls[-1][1][9] == 0.5 and spy.calls[-1][1][10] is False
    n = len(spy.calls)
    for kw, text in ((dict(), "block_table=None is not implemented"), (dict(block_table=table, dropout_p=0.1), "dropout_p"),
                     (dict(block_table=table, window_size=(128, 0)), "window_size=\\(128, 0\\)"), (dict(block_table=table, softcap=30.0), "softcap=30.0"),
                     (dict(block_table=table, alibi_slopes=torch.zeros(8)), "alibi_slopes=tensor\\(8,\\)"),
                     (dict(block_table=table, return_attn_probs=True), "return_attn_probs=True"),
                     (dict(block_table=table, seqused_k=torch.zeros(2)), "seqused_k")):
        with pytest.raises(NotImplementedError, match=text):
            F.flash_attn_varlen_func(q, pool, pool, cu_q, cu_k, 40, 192, **kw)
    assert len(spy.calls) == n
    # flash_attn_with_kvcache is unchanged: a block table is still refused there
    with pytest.raises(NotImplementedError, match="block_table"):
        F.flash_attn_with_kvcache(torch.zeros(2, 4, 8, 128, dtype=torch.float16), pool, pool, cache_seqlens=3, block_table=table)


# ------------------------------------------------------------------------------------------------------------------------
# the packed batches are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_the_axes_of_the_issue():
    names = {s["name"] for s in V.CASES}
    assert len(names) == len(V.CASES) and len(V.PAGED_CASES) == 2 * len(V.CASES)
    assert (V.H, V.HKV, V.BOUND, V.PAGE_SIZES) == (8, 2, 384, (64, 128)) and V.PAD_ROWS == 5 and V.PAD_COLS > 0
    assert V.MIXED_SQ == (1, 33, 0, 64, 65, 130, 1, 17)
    for tag in ("mixed", "loose", "over", "short", "full", "uniform"):
        mine = [s for s in V.CASES if s["name"].startswith(tag)]
        assert {s["Dh"] for s in mine} == {64, 128} and {s["dtype"] for s in mine} == {torch.float16, torch.bfloat16}, tag
    mixed = [s for s in V.CASES if s["name"].startswith("mixed")]
    assert {s["mode"] for s in mixed} == {"diag", "scatter", "edges", "negscale", "pair", "decoy"} and all(s["max_q"] == 130 for s in mixed)
    vb = V.VarqBatch(mixed[0])
    assert vb.seqlens_k.tolist() == [191, 0, 64, 31, 63, 127, -1, V.BOUND + 1 - 17] and vb.total() == [192, 33, 64, 95, 128, 257, 0, V.BOUND + 1]
    assert vb.cu == [0, 1, 34, 34, 98, 163, 293, 294, 311] and vb.total_q == 316 and torch.isnan(vb.q[311:]).all()
    assert not torch.isnan(vb.q[:311]).any() and (vb.expect[311:] == V.SENTINEL).all() and not vb.expect[293:311].any()
    assert [vb.active(b) for b in range(8)] == [True] * 6 + [False, False] and torch.isnan(vb.k_cache[6:]).all()
    assert not torch.isnan(vb.k_cache[2, :64]).any() and torch.isnan(vb.k_cache[2, 64:]).all()      # the idle slot keeps its 64 keys
    loose = V.VarqBatch(next(s for s in V.CASES if s["name"].startswith("loose-diag") and s["dtype"] == vb.dtype))
    assert loose.max_q == 256 and loose.cu == vb.cu
    over = V.VarqBatch(next(s for s in V.CASES if s["name"].startswith("over")))
    assert over.sq[1] == 70 > over.max_q == 64 and not over.active(1) and not over.expect[40:104].any()
    assert (over.expect[104:110] == V.SENTINEL).all() and torch.isnan(over.k_cache[1]).all()
    short = V.VarqBatch(next(s for s in V.CASES if s["name"].startswith("short")))
    assert not short.before and sum(n < q for n, q in zip(short.lens, short.sq) if n > 0) == 3
    assert not short.expect[:45].any() and short.expect[45:65].any()
    assert sum(not s.get("causal", True) for s in V.CASES) == 4
    uni = [s for s in V.CASES if s["name"].startswith("uniform")]
    assert all(set(s["sq"]) == {65} and s["max_q"] == 65 for s in uni)
    pp = V.PagedVarq(V.PAGED_CASES[0])
    assert pp.table_full.stride(0) == pp.pps + V.PAD_COLS and pp.table.stride(0) > pp.table.shape[1]


@pytest.mark.parametrize("spec", V.CASES, ids=V.case_id)
def test_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    vb = V.VarqBatch(spec)
    for b in range(len(vb.sq)):  # every cache row that holds no key is NaN
        held = vb.held(b)
        assert not torch.isnan(vb.k_cache[b, :held]).any() and torch.isnan(vb.k_cache[b, held:]).all() and torch.isnan(vb.v_cache[b, held:]).all()
    assert torch.equal(bits(V.attend(vb)), bits(vb.expect))
    for mutant in V.ATTN_MUTANTS:
        if V.attn_mutant_applies(vb, mutant):
            assert not torch.equal(bits(V.attend(vb, mutant)), bits(vb.expect)), mutant
    if vb.before:
        assert V.store_map(vb) == V.store_expect(vb)
        for mutant in V.STORE_MUTANTS:
            if V.store_mutant_applies(vb, mutant):
                assert V.store_map(vb, mutant) != V.store_expect(vb), mutant


@pytest.mark.parametrize("spec", [s for s in V.PAGED_CASES if s["dtype"] == torch.float16], ids=V.case_id)
def test_paged_restatement_returns_the_targets(spec):
    pp = V.PagedVarq(spec)  # (asserts the gather and the NaN of every row that holds no key)
    assert torch.equal(bits(V.attend(pp.batch, pp=pp)), bits(pp.batch.expect))


def test_every_mutant_is_seen_by_some_batch():
    seen = {m: 0 for m in V.ATTN_MUTANTS + V.STORE_MUTANTS}
    for spec in V.CASES:
        if spec["dtype"] == torch.float16:
            vb = V.VarqBatch(spec)
            for m in V.ATTN_MUTANTS:
                seen[m] += V.attn_mutant_applies(vb, m)
            for m in V.STORE_MUTANTS:
                seen[m] += vb.before and V.store_mutant_applies(vb, m)
    assert all(v > 0 for v in seen.values()), seen
