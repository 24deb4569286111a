"""Attention over the KV cache with device-side lengths, without a GPU: the six exports, the host plan made from a bound, the workspace
formula, every argument check of the C ABI, the flash_attn_with_kvcache shim's keyword handling, and the soundness of the ragged needle
batches of tests/attn_kvcache_cases.py -- the list tests/test_gpu_attention_kvcache.py runs through the kernels -- against the torch
restatement of the ragged call and each of its mutants."""
import ctypes
import os

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_kvcache_cases as K

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
SYMBOLS = ("awq_rope_kv_store_natural_pos", "awq_rope_kv_store_natural_pos_fp8", "awq_attn_kvcache", "awq_attn_kvcache_kv8",
           "awq_attn_kvcache_plan", "awq_attn_kvcache_workspace_bytes")


def test_library_engine_ops_and_shim_export_the_kvcache_surface():
    L = _capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params(eng.attn_kvcache) == ["q", "k_cache", "v_cache", "seqlens_k", "max_seqlen_k", "seqlen_offset", "softmax_scale", "causal"]
    assert params(eng.attn_kvcache_kv8) == ["q", "k_cache", "v_cache", "k_scale", "v_scale", "seqlens_k", "max_seqlen_k", "seqlen_offset",
                                            "softmax_scale", "causal"]
    assert params(eng.attn_kvcache_plan) == ["batch", "nheads", "nheads_kv", "head_dim", "seqlen_q", "max_seqlen_k"]
    assert params(eng.rope_kv_store_natural_pos) == ["qkv", "freqs_table", "k_cache", "v_cache", "cache_seqlens", "nheads", "nheads_kv"]
    assert params(eng.rope_kv_store_natural_pos_fp8) == ["qkv", "freqs_table", "k_cache", "v_cache", "k_scale", "v_scale", "cache_seqlens",
                                                         "nheads", "nheads_kv"]
    for name in ("attn_kvcache_plan", "attn_kvcache", "rope_kv_store_natural_pos"):
        assert callable(getattr(ops, name)), name
    assert eng.attn_kvcache_plan(1, 32, 8, 128, 1, 32768) == ops.attn_kvcache_plan(1, 32, 8, 128, 1, 32768)
    mod = llm_awq_amd.install_as_flash_attn()
    from llm_awq_amd import flash_attn_compat as F
    if mod is F:  # (a real flash_attn package is left alone)
        from flash_attn import flash_attn_with_kvcache
        from flash_attn.flash_attn_interface import flash_attn_with_kvcache as again
        assert flash_attn_with_kvcache is F.flash_attn_with_kvcache is again


# ------------------------------------------------------------------------------------------------------------------------
# the plan: made from the bound alone
# ------------------------------------------------------------------------------------------------------------------------
MODELS = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128), "qwen2_7b": (28, 4, 128), "llama3_70b_tp8": (8, 1, 128), "small": (8, 2, 64)}
GRID = [(m, B, Sq, bound) for m in sorted(MODELS) for B in (1, 3, 8, 64) for Sq in (1, 4) for bound in (1, 100, 1024, 1025, 2304, 32768, 131072)]


def _ws(B, H, Hkv, Dh, Sq, bound):
    return _capi.lib().awq_attn_kvcache_workspace_bytes(B, H, Hkv, Dh, Sq, bound)


@pytest.mark.parametrize("model,B,Sq,bound", GRID, ids=lambda x: str(x))
def test_plan_covers_the_bound_and_the_workspace_follows(model, B, Sq, bound):
    H, Hkv, Dh = MODELS[model]
    splits, chunk = ops.attn_kvcache_plan(B, H, Hkv, Dh, Sq, bound)
    assert splits >= 1 and chunk % 64 == 0 and chunk >= 1024
    assert (splits - 1) * chunk < bound <= splits * chunk
    if bound <= 1024:
        assert splits == 1
    if Hkv * (bound // 1024) >= 512:  # two blocks per CU for ONE sequence at the bound wherever the 1024-key floor allows
        assert Hkv * splits >= 256
    assert (splits, chunk) == ops.attn_kvcache_plan(1, H, Hkv, Dh, Sq, bound)  # the batch does not enter: any of its sequences may be the only long one
    assert _ws(B, H, Hkv, Dh, Sq, bound) == B * H * Sq * splits * (Dh + 2) * 4 > 0


def test_plan_pins():
    assert ops.attn_kvcache_plan(1, 8, 2, 128, 1, 100) == (1, 1024)               # one split: the pair still runs
    assert ops.attn_kvcache_plan(3, 8, 2, 64, 1, 2304) == (3, 1024)               # the random shapes of the GPU tests
    assert ops.attn_kvcache_plan(3, 8, 2, 128, 4, 2304) == (3, 1024)
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 2048) == (2, 1024)             # no 2048-key floor, no one-pass test
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 131072) == (64, 2048)          # the host-length plan's chunk at the same length
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 131072)[1] == ops.attn_splitkv_plan(1, 32, 8, 128, 1, 131072, True)[1]
    assert ops.attn_kvcache_plan(8, 32, 8, 128, 1, 131072) == (64, 2048)          # sized for one sequence, whatever the batch
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 8192) == ops.attn_splitkv_plan(1, 32, 8, 128, 1, 8192, True) == (8, 1024)
    # the plan takes no length: six host ints, of which the bound is the only one that speaks of keys, and the two results
    args = _capi.SIGNATURES["awq_attn_kvcache_plan"][1]
    assert args[:6] == [ctypes.c_int] * 6 and args[6:] == [ctypes.POINTER(ctypes.c_int)] * 2
    assert _capi.SIGNATURES["awq_attn_kvcache_workspace_bytes"][1] == [ctypes.c_int] * 6


def test_plan_refuses_what_the_split_kernels_do_not_serve():
    L = _capi.lib()
    s, c = ctypes.c_int(), ctypes.c_int()
    ok = (1, 32, 8, 128, 1, 4096)
    assert L.awq_attn_kvcache_plan(*ok, ctypes.byref(s), ctypes.byref(c)) == 0
    for bad in ((0, 32, 8, 128, 1, 4096), (1, 0, 8, 128, 1, 4096), (1, 32, 0, 128, 1, 4096), (1, 32, 6, 128, 1, 4096), (1, 32, 8, 96, 1, 4096),
                (1, 32, 8, 72, 1, 4096), (1, 32, 8, 128, 0, 4096), (1, 32, 8, 128, 33, 4096), (1, 32, 8, 128, 1, 0), (1, 32, 8, 128, 1, -5)):
        assert L.awq_attn_kvcache_plan(*bad, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE, bad
        assert L.awq_attn_kvcache_workspace_bytes(*bad) == 0, bad
    assert L.awq_attn_kvcache_plan(1, 32, 8, 128, 32, 4096, ctypes.byref(s), ctypes.byref(c)) == 0  # Sq * G = 128: the last shape served
    assert L.awq_attn_kvcache_plan(*ok, None, ctypes.byref(c)) == AWQ_ERR_NULL
    assert L.awq_attn_kvcache_plan(*ok, ctypes.byref(s), None) == AWQ_ERR_NULL


@pytest.fixture
def knob():
    had = os.environ.get("AWQ_TUNING")
    yield lambda c: _capi.tune(attn_splitkv_chunk=c)
    _capi.tune(attn_splitkv_chunk=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def test_plan_follows_the_knob(knob):
    before = ops.attn_kvcache_plan(1, 32, 8, 128, 1, 32768)
    knob(64)
    assert ops.attn_kvcache_plan(1, 8, 2, 128, 1, 257) == (5, 64)
    assert ops.attn_kvcache_plan(1, 8, 2, 128, 1, 1024) == (16, 64)
    assert ops.attn_kvcache_plan(1, 8, 2, 128, 8, 64) == (1, 64)
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 32768) == (512, 64)
    assert _ws(6, 8, 2, 128, 1, 257) == 6 * 8 * 1 * 5 * 130 * 4
    knob(4096)
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 32768) == (8, 4096)
    knob(0)
    assert ops.attn_kvcache_plan(1, 32, 8, 128, 1, 32768) == before


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


ATTN_OK = dict(B=2, Sq=1, off=1, bound=4096, lmax=4100, H=8, Hkv=2, Dh=128, qbs=1024, qrs=1024, kbs=4100 * 256, krs=256, vbs=4100 * 256, vrs=256,
               ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0)


def _attn(p, kv8=False, **kw):
    """The workspace stays NULL unless a test gives one, so even a call that passes every other check launches nothing."""
    a = dict(ATTN_OK, q=p, k=p, v=p, ks=p, vs=p, out=p, lens=p, ws=None, wsb=0)
    a.update(kw)
    L = _capi.lib()
    head = (a["B"], a["Sq"], a["lens"], a["off"], a["bound"], a["lmax"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"], a["kbs"], a["krs"], a["vbs"],
            a["vrs"])
    tail = (a["scale"], a["causal"], a["dtype"], a["ws"], a["wsb"], None)
    if kv8:
        return L.awq_attn_kvcache_kv8(a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], *head, a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"], *tail)
    return L.awq_attn_kvcache(a["q"], a["k"], a["v"], a["out"], *head, *tail)


@pytest.mark.parametrize("kv8", [False, True], ids=["T", "kv8"])
def test_attn_kvcache_argument_validation_returns_codes_without_launch(kv8):
    buf, p = _p16()
    for bad in (dict(Dh=32), dict(Dh=96), dict(Dh=72), dict(Dh=256), dict(H=6, Hkv=4), dict(B=0), dict(Sq=0), dict(H=0), dict(Hkv=0),
                dict(Sq=33), dict(Sq=129), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8), dict(kbs=-256), dict(vbs=-256),
                dict(bound=0), dict(bound=-1), dict(bound=4101), dict(off=-1)):
        assert _attn(p, kv8, **bad) == AWQ_ERR_SHAPE, bad
    assert _attn(p, kv8, Sq=32) == AWQ_ERR_WORKSPACE   # Sq * G = 128 is served
    assert _attn(p, kv8, bound=4100) == AWQ_ERR_WORKSPACE  # the bound may equal the cache length
    assert _attn(p, kv8, causal=0) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "lens") + (("ks", "vs") if kv8 else ()):
        assert _attn(p, kv8, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):
        assert _attn(p, kv8, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _attn(p, kv8, lens=p + 2) == AWQ_ERR_ALIGN
    assert _attn(p, kv8, lens=p + 4) == AWQ_ERR_WORKSPACE  # four bytes are enough for the lengths
    if kv8:
        assert _attn(p, kv8, ks=p + 2) == AWQ_ERR_ALIGN and _attn(p, kv8, vs=p + 2) == AWQ_ERR_ALIGN
        assert _attn(p, kv8, ksrs=1) == AWQ_ERR_SHAPE and _attn(p, kv8, vsrs=1) == AWQ_ERR_SHAPE
        assert _attn(p, kv8, ksbs=-2) == AWQ_ERR_SHAPE and _attn(p, kv8, vsbs=-2) == AWQ_ERR_SHAPE
        for name, val in (("kbs", 4100 * 256 + 8), ("krs", 264), ("vbs", 4100 * 256 + 8), ("vrs", 264)):  # strides in codes: multiples of 16
            assert _attn(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 1028), ("qrs", 1028), ("kbs", 4100 * 256 + 4), ("krs", 260), ("vbs", 4100 * 256 + 4), ("vrs", 260)):
        assert _attn(p, kv8, **{name: val}) == AWQ_ERR_ALIGN, name
    need = _ws(2, 8, 2, 128, 1, 4096)
    assert need == 2 * 8 * 1 * ops.attn_kvcache_plan(2, 8, 2, 128, 1, 4096)[0] * 130 * 4 > 0
    assert _attn(p, kv8) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, ws=None, wsb=need) == AWQ_ERR_WORKSPACE
    assert _attn(p, kv8, ws=p + 4, wsb=need) == AWQ_ERR_ALIGN
    # one split needs its workspace too: the pair always runs
    assert _attn(p, kv8, bound=100, lmax=100, kbs=100 * 256, vbs=100 * 256) == AWQ_ERR_WORKSPACE


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_store_pos_argument_validation_returns_codes_without_launch(fp8):
    """Every call here is refused: a call that passed would launch, and there is no GPU."""
    buf, p = _p16()
    L = _capi.lib()
    ok = dict(qkv=p, fr=p, q=p, kc=p, vc=p, ks=p, vs=p, lens=p, B=1, Bc=2, S=4, H=8, Hkv=2, Dh=128, rot=128, lmax=64, rows=64, bs=4 * 1536,
              rs=1536, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        tail = (a["lens"], a["B"], a["Bc"], a["S"], a["H"], a["Hkv"], a["Dh"], a["rot"], a["lmax"], a["rows"], a["bs"], a["rs"], a["dtype"], None)
        if fp8:
            return L.awq_rope_kv_store_natural_pos_fp8(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], a["ks"], a["vs"], *tail)
        return L.awq_rope_kv_store_natural_pos(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], *tail)
    for bad in (dict(Dh=96), dict(Dh=72), dict(rot=24), dict(rot=144), dict(rot=0), dict(B=3), dict(B=0), dict(S=0), dict(H=0), dict(Hkv=0),
                dict(lmax=0), dict(rows=0), dict(rows=-1), dict(rs=1528), dict(bs=-8)):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    assert call(dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "fr", "q", "kc", "vc", "lens") + (("ks", "vs") if fp8 else ()):
        assert call(**{name: None}) == AWQ_ERR_NULL, name
    for name in ("qkv", "fr", "q", "kc", "vc"):
        assert call(**{name: p + 4}) == AWQ_ERR_ALIGN, name
    assert call(lens=p + 2) == AWQ_ERR_ALIGN
    if fp8:
        assert call(ks=p + 2) == AWQ_ERR_ALIGN and call(vs=p + 2) == AWQ_ERR_ALIGN
    assert call(bs=4 * 1536 + 4) == AWQ_ERR_ALIGN and call(rs=1540) == AWQ_ERR_ALIGN


def test_flash_attn_with_kvcache_names_what_it_does_not_serve():
    from llm_awq_amd import flash_attn_compat as F

    q = torch.zeros(2, 1, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    lens = torch.tensor([5, 9], dtype=torch.int32)
    new = torch.zeros(2, 1, 2, 128, dtype=torch.float16)
    for kw, word in ((dict(k=new, v=new), "k="), (dict(v=new), "v="), (dict(rotary_cos=torch.ones(4, 64)), "rotary_cos"),
                     (dict(rotary_sin=torch.ones(4, 64)), "rotary_sin"), (dict(block_table=torch.zeros(2, 4, dtype=torch.int32)), "block_table"),
                     (dict(cache_batch_idx=torch.zeros(2, dtype=torch.int32)), "cache_batch_idx"), (dict(window_size=(128, 0)), "window_size"),
                     (dict(softcap=30.0), "softcap"), (dict(alibi_slopes=torch.ones(8)), "alibi_slopes"),
                     (dict(cache_leftpad=torch.zeros(2, dtype=torch.int32)), "cache_leftpad"), (dict(return_softmax_lse=True), "return_softmax_lse")):
        with pytest.raises(NotImplementedError, match=word):
            F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=lens, causal=True, **kw)
    # a served call reaches the engine, which refuses CPU tensors: not a NotImplementedError, and not a silent torch fallback
    for served in (dict(cache_seqlens=lens), dict(cache_seqlens=7), dict(cache_seqlens=None), dict(cache_seqlens=lens, window_size=(-1, -1), softcap=0.0)):
        with pytest.raises(RuntimeError, match="GPU") as e:
            F.flash_attn_with_kvcache(q, kc, kc, causal=True, **served)
        assert not isinstance(e.value, NotImplementedError)


def test_ft_layout_refuses_a_tensor_start_pos_before_any_work():
    from types import SimpleNamespace

    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused

    class Boom(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the projection must not run")
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0)
    m = QuantLlamaAttentionFused(512, 8, 64, Boom(), Boom(), "cpu", args, max_batch_size=2, kv_layout="ft")
    with pytest.raises(ValueError, match="natural"):
        m(torch.zeros(2, 1, 512), torch.zeros(2, dtype=torch.int32), torch.zeros(64, 64))


# ------------------------------------------------------------------------------------------------------------------------
# the needle batches are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_axes_of_the_issue():
    names = {s["name"] for s in K.CASES}
    assert len(names) == len(K.CASES)
    assert {(s["Sq"], s["lens"], s["bound"]) for s in K.CASES} == set(K.SHAPES)
    assert K.SHAPES == ((1, (65, 129, 1, 64, 257, None), 257), (1, (65, 129, 1, 64, 257, None), 1024), (8, (193, 8, 72, 257, 9), 257),
                        (32, (257, 32, 100, 33), 257))
    assert {s["H"] // s["Hkv"] for s in K.CASES} == {1, 4, 8} and {s["Hkv"] for s in K.CASES} == {1, 2}
    assert {s["Dh"] for s in K.CASES} == {64, 128} and {s["dtype"] for s in K.CASES} == {torch.float16, torch.bfloat16}
    assert all(s["Sq"] * (s["H"] // s["Hkv"]) <= 128 for s in K.CASES)
    assert all(s["H"] // s["Hkv"] <= 4 for s in K.CASES if s["Sq"] == 32)
    for shape in K.SHAPES:
        mine = [s for s in K.CASES if (s["Sq"], s["lens"], s["bound"]) == shape]
        want = {"diag", "scatter", "edges", "negscale", "pair"} | ({"decoy"} if shape[0] > 1 else set())
        assert {s["mode"] for s in mine} == want, shape
        assert {s["Dh"] for s in mine} == {64, 128} and {s["Hkv"] for s in mine} == {1, 2} and len({s["H"] // s["Hkv"] for s in mine}) > 1
        assert {s["offset"] for s in mine} == ({shape[0], 0} if None not in shape[1] else {1, 0})


@pytest.mark.parametrize("spec", K.CASES, ids=K.case_id)
def test_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    batch = K.Batch(spec)
    assert batch.total() == [n if n is not None else batch.offset - 1 for n in batch.lens]
    assert not torch.isnan(batch.q).any()
    for b, n in enumerate(batch.lens):  # NaN wherever the cache holds no key
        n = n or 0
        assert not torch.isnan(batch.k_cache[b, :n]).any() and not torch.isnan(batch.v_cache[b, :n]).any()
        assert torch.isnan(batch.k_cache[b, n:]).all() and torch.isnan(batch.v_cache[b, n:]).all()
    for chunk in (K.CHUNK, 128, 1024):  # the targets do not depend on how the keys are cut
        out = K.ragged(batch, chunk=chunk)
        assert torch.equal(out.view(torch.int16), batch.target.view(torch.int16)), chunk
    for b, n in enumerate(batch.lens):
        if n is None:
            assert not batch.target[b].any()
    for mutant in K.MUTANTS:
        if not K.mutant_applies(batch, mutant):
            continue
        bad = K.ragged(batch, mutant=mutant)
        assert not torch.equal(bad.view(torch.int16), batch.target.view(torch.int16)), mutant


def test_every_mutant_is_seen_by_some_batch_of_every_shape_it_can_show_at():
    for shape in K.SHAPES:
        seen = {m: 0 for m in K.MUTANTS}
        for spec in K.CASES:
            if (spec["Sq"], spec["lens"], spec["bound"]) == shape:
                batch = K.Batch(spec)
                for m in K.MUTANTS:
                    seen[m] += K.mutant_applies(batch, m)
        cannot = set()
        if shape[0] == 1:
            cannot.add("shiftmax")      # one query row attends every key it is given, whatever the shift
        if None not in shape[1]:
            cannot.add("inactive-nan")  # no inactive row in the batch
        assert all(v > 0 for m, v in seen.items() if m not in cannot), (shape, seen)
