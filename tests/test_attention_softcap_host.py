"""Soft-capped attention on packed steps, without a GPU: the oracle against the window oracle and a case by hand, every oracle mutant seen
by the step of tests/attn_softcap_cases.py (the table below, computed from the float64 oracle alone), the exports at every layer, the
refusals of the four C entries and of ops.attn_varq_softcap before any launch, and the module: what it routes where, what it leaves as it
was and what it refuses."""
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_softcap_cases as C
from tests import attn_softcap_oracle as O
from tests import attn_window_oracle as WO

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
ENTRIES = ("awq_attn_varq_softcap", "awq_attn_varq_softcap_kv8", "awq_attn_paged_varq_softcap", "awq_attn_paged_varq_softcap_kv8")
WINDOWED = ("awq_attn_varq_window", "awq_attn_varq_window_kv8", "awq_attn_paged_varq_window", "awq_attn_paged_varq_window_kv8")
I, VP, SZ, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------
def test_the_derived_constant_meets_the_condition():
    assert O.C <= 16
    # the two facts the derivation leans on: max x sech^2(x) and the rounding of 2 log2 e to fp32
    x = torch.linspace(0, 20, 2_000_001, dtype=torch.float64)
    assert float((x / torch.cosh(x) ** 2).max()) < 0.4478
    k32 = float(torch.tensor(2.8853900817779268, dtype=torch.float32))
    assert abs(k32 - 2 * O.LOG2E) / (2 * O.LOG2E) <= 0.7 * 2.0 ** -24


def test_oracle_without_a_cap_is_the_window_oracle():
    g = torch.Generator().manual_seed(5)
    q, k, v = torch.randn(2, 9, 4, 64, generator=g), torch.randn(2, 40, 2, 64, generator=g), torch.randn(2, 40, 2, 64, generator=g)
    for left in (0, 5, 39):
        want = WO.attention(q, k, v, left, stats=True)
        got = O.attention(q, k, v, left, INF, stats=True)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        big = O.attention(q, k, v, left, 1e9)                       # cap -> inf: tanh(y) -> y
        assert torch.allclose(big, want[0], rtol=0, atol=1e-12)
        want = WO.attention(q, k, v, left, scale=0.31)
        assert torch.equal(O.attention(q, k, v, left, INF, scale=0.31), want)
    ref, A, qk = O.attention(q, k, v, 5, INF, stats=True)
    assert torch.equal(O.bound(ref, A, qk, torch.float16, 40, 64, 0.125, INF), O.P.bound(ref, A, qk, torch.float16, 40, 64, 0.125))
    grown = O.bound(ref, A, qk, torch.float16, 40, 64, 0.125, 50.0) - O.P.bound(ref, A, qk, torch.float16, 40, 64, 0.125)
    assert torch.allclose(grown, 2 * O.C * 2.0 ** -24 * 50.0 * A, rtol=1e-9, atol=0)


@pytest.mark.parametrize("cap", [2.0, 30.0, 50.0])
def test_two_keys_by_hand(cap):
    """Scores +- cap * atanh(0.5): the capped logits are +- cap / 2 and the weights e^(cap / 2) : e^(-cap / 2)."""
    s = cap * math.atanh(0.5)
    q = torch.zeros(1, 1, 1, 64, dtype=torch.float64)
    q[0, 0, 0, 0] = 1.0
    k = torch.zeros(1, 2, 1, 64, dtype=torch.float64)
    k[0, 0, 0, 0], k[0, 1, 0, 0] = s, -s
    v = torch.zeros(1, 2, 1, 64, dtype=torch.float64)
    v[0, 0, 0, :], v[0, 1, 0, :] = 1.0, -1.0
    out = O.attention(q, k, v, 1, cap, scale=1.0)
    w0 = math.exp(cap / 2) / (math.exp(cap / 2) + math.exp(-cap / 2))
    assert torch.allclose(out, torch.full_like(out, 2 * w0 - 1), rtol=1e-12, atol=1e-15)
    # the mask behind the cap: with window_left 0 the row attends key 1 alone, weight exactly 1 -- -cap would leave key 0 e^(-cap/2 .. ) of it
    assert torch.equal(O.attention(q, k, v, 0, cap, scale=1.0), torch.full_like(out, -1.0))
    leaked = O.attention(q, k, v, 0, cap, scale=1.0, mutant="cap-after-mask")
    # key 1 (v = -1) at -cap / 2 against the masked key 0 (v = +1) at -cap
    assert torch.allclose(leaked, torch.full_like(out, -(math.exp(-cap / 2) - math.exp(-cap)) / (math.exp(-cap / 2) + math.exp(-cap))), rtol=1e-9)
    # a dead key contributes exactly nothing, whatever it holds
    k[0, 0, 0, :], v[0, 0, 0, :] = NAN, NAN
    assert torch.equal(O.attention(q, k, v, 0, cap, scale=1.0), torch.full_like(out, -1.0))


# ------------------------------------------------------------------------------------------------------------------------
# the step sees every mutant: the table, from the float64 oracle alone
# ------------------------------------------------------------------------------------------------------------------------
_ST, _SEEN = {}, {}
TABLE_COMBOS = ((torch.bfloat16, 128), (torch.float16, 64))
VALUE_MUTANTS = ("nocap", "scale-outside", "log2e-inside", "half-arg")


def _seen(dtype, Dh, left, cap):
    """{mutant: the active sequences on which some element of the mutant lies beyond the bound of the truth}"""
    key = (dtype, Dh, left, cap)
    if key not in _SEEN:
        st = _ST.get((dtype, Dh)) or _ST.setdefault((dtype, Dh), C.Step(dtype, Dh))
        res = {m: set() for m in O.MUTANTS}
        for b, (n, h) in enumerate(C.STEP):
            if not C.active_rows(b):
                continue
            q, k, v = st.seq(b)
            ref, A, qk = O.attention(q, k, v, left, cap, stats=True)
            bound = O.bound(ref, A, qk, dtype, h + n, Dh, Dh ** -0.5, cap)
            for m in O.MUTANTS:
                if cap == 50.0 and m == "cap-after-mask":
                    continue                                         # e^-50: below any bound, never asked for
                if bool(((O.attention(q, k, v, left, cap, mutant=m) - ref).abs() > bound).any()):
                    res[m].add(b)
        _SEEN[key] = res
    return _SEEN[key]


@pytest.mark.parametrize("left", C.LEFTS)
@pytest.mark.parametrize("dtype,Dh", TABLE_COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_the_step_tells_every_mutant_from_the_oracle(dtype, Dh, left):
    everyone = {b for b in range(len(C.STEP)) if C.active_rows(b)}
    assert everyone == {0, 1, 2, 3, 7, 8, 9}
    for cap in C.CAPS:
        seen = _seen(dtype, Dh, left, cap)
        for m in VALUE_MUTANTS:
            assert seen[m], (cap, m)                                 # each of the four, at every cap
            if cap in (2.0, 5.0):
                assert seen[m] == everyone, (cap, m, seen[m])        # ... on every active sequence
        if cap == 50.0:
            assert {1, 2, 3} <= seen["nocap"], seen["nocap"]
    assert _seen(dtype, Dh, left, 2.0)["cap-after-mask"], "a masked key at -cap is seen at cap 2"


def test_left_0_sees_no_value_mutant():
    st = _ST.get((torch.float16, 64)) or _ST.setdefault((torch.float16, 64), C.Step(torch.float16, 64))
    q, k, v = st.seq(1)
    ref = O.attention(q, k, v, 0, 2.0)
    for m in VALUE_MUTANTS:
        assert torch.equal(O.attention(q, k, v, 0, 2.0, mutant=m), ref), m


# ------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------
def test_library_header_engine_and_ops_export_the_cap():
    L = ctypes.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "awq_attn_varq_window_plan / awq_attn_varq_window_workspace_bytes" in header     # the header names the plan of the capped entries
    assert _capi.lib().awq_abi_version() == 1      # symbols were added, none changed
    S_ = _capi.SIGNATURES
    for new, old in zip(ENTRIES, WINDOWED):        # the windowed entry's arguments with softcap directly behind window_left
        assert list(S_[new][1]) == list(S_[old][1])[:-3] + [F, VP, SZ, VP] and S_[old][1][-4] is I, new
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    tail = ["cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "split_seqlen_q", "split_min_keys", "window_left", "softcap",
            "lens_before_step", "softmax_scale", "causal", "out"]
    assert params(eng.attn_varq_softcap) == ["q", "k_cache", "v_cache"] + tail
    assert params(eng.attn_varq_softcap_kv8) == ["q", "k_cache", "v_cache", "k_scale", "v_scale"] + tail
    assert params(eng.attn_paged_varq_softcap) == ["q", "k_pool", "v_pool", "block_table"] + tail
    assert params(eng.attn_paged_varq_softcap_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table"] + tail
    # a function of its own: ops.attn_varq and ops.attn_varq_window keep their parameter lists
    assert list(inspect.signature(ops.attn_varq_softcap).parameters) == [
        "q", "k", "v", "cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "softcap", "window_left", "split_seqlen_q", "split_min_keys",
        "lens_before_step", "block_table", "softmax_scale", "causal", "k_scale", "v_scale", "out"]
    sig = inspect.signature(ops.attn_varq_softcap).parameters
    assert sig["softcap"].default is inspect.Parameter.empty and sig["window_left"].default is None
    assert "softcap" not in inspect.signature(ops.attn_varq).parameters and "softcap" not in inspect.signature(ops.attn_varq_window).parameters
    from llm_awq_amd import flash_attn_compat, fused_attn

    init = inspect.signature(fused_attn.QuantLlamaAttentionFused.__init__).parameters
    assert list(init)[-2:] == ["attn_softcap", "softmax_scale"] and init["attn_softcap"].default is None and init["softmax_scale"].default is None
    assert list(inspect.signature(fused_attn.make_quant_attn_softcap).parameters) == [
        "model", "dev", "attn_softcap", "softmax_scale", "sliding_window", "max_batch_size", "kv_layout", "kv_dtype"]
    assert "attn_softcap" not in inspect.signature(fused_attn.make_quant_attn).parameters
    assert "softcap" in inspect.signature(flash_attn_compat.flash_attn_with_kvcache).parameters     # ... which keeps refusing it


# ------------------------------------------------------------------------------------------------------------------------
# argument validation of the four entries: every call here is refused, no launch
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


OK = dict(B=3, maxq=512, total=700, before=1, bound=4096, lmax=4100, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qrs=1024,
          kbs=4100 * 256, krs=256, vbs=4100 * 256, vrs=256, ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0,
          sq=1, floor=2048, left=1023, cap=50.0, wsb=1 << 40)


def _call(p, paged, kv8, **kw):
    a = dict(OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, cu=p, lens=p, ws=p)
    if paged:
        a.update(kbs=256 * 256, vbs=256 * 256, ksbs=512, vsbs=512)
    a.update(kw)
    step = (a["B"], a["cu"], a["maxq"], a["total"], a["lens"], a["before"], a["bound"])
    where = (a["bt"], *step, a["pages"], a["ps"], a["pps"], a["trs"]) if paged else (*step, a["lmax"])
    strides = (a["qrs"], a["kbs"], a["krs"], a["vbs"], a["vrs"]) + ((a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"]) if kv8 else ())
    fn = getattr(_capi.lib(), "awq_attn_" + ("paged_" if paged else "") + "varq_softcap" + ("_kv8" if kv8 else ""))
    return fn(a["q"], a["k"], a["v"], *((a["ks"], a["vs"]) if kv8 else ()), a["out"], *where, a["H"], a["Hkv"], a["Dh"], *strides, a["scale"],
              a["causal"], a["dtype"], a["sq"], a["floor"], a["left"], a["cap"], a["ws"], a["wsb"], None)


FORMS = [(False, False), (False, True), (True, False), (True, True)]
FORM_IDS = ["dense-T", "dense-fp8", "paged-T", "paged-fp8"]


@pytest.mark.parametrize("paged,kv8", FORMS, ids=FORM_IDS)
def test_entries_refuse_without_a_launch(paged, kv8):
    buf, p = _p16()
    need = _capi.lib().awq_attn_varq_window_workspace_bytes(3, 8, 2, 128, 1, 4096, 1023)
    assert need > 0
    # the cap's own terms: below 0, infinite, NaN -- refused in the shape phase, before the alignment of the lengths and the workspace
    for bad in (-1.0, -1e-30, -INF, INF, NAN):
        assert _call(p, paged, kv8, cap=bad) == AWQ_ERR_SHAPE, bad
        assert _call(p, paged, kv8, cap=bad, lens=p + 2, ws=None) == AWQ_ERR_SHAPE, bad
    # the siblings' terms stay, with a cap and with cap = 0
    for cap in (50.0, 0.0):
        for bad in (dict(left=-1), dict(causal=0), dict(sq=-1), dict(floor=0), dict(sq=33), dict(maxq=0), dict(total=0), dict(B=0), dict(B=65536),
                    dict(Dh=96), dict(H=6, Hkv=4), dict(qrs=512), dict(krs=128), dict(bound=0), dict(bound=4097) if paged else dict(bound=4101)):
            assert _call(p, paged, kv8, cap=cap, **bad) == AWQ_ERR_SHAPE, (cap, bad)
        # what passes the shape phase reaches the alignment phase and, behind it, the WINDOW's workspace
        for ok in (dict(left=0), dict(left=4095), dict(left=2 ** 31 - 1), dict(sq=0), dict(sq=32, left=5)):
            assert _call(p, paged, kv8, cap=cap, cu=p + 2, **ok) == AWQ_ERR_ALIGN, ok
            assert _call(p, paged, kv8, cap=cap, lens=p + 2, **ok) == AWQ_ERR_ALIGN, ok
            if ok.get("sq", 1) > 0:
                assert _call(p, paged, kv8, cap=cap, ws=None, **ok) == AWQ_ERR_WORKSPACE, ok
        assert _call(p, paged, kv8, cap=cap, wsb=need - 1) == AWQ_ERR_WORKSPACE
        assert _call(p, paged, kv8, cap=cap, wsb=need, ws=p + 4) == AWQ_ERR_ALIGN
        assert _call(p, paged, kv8, cap=cap, dtype=2) == AWQ_ERR_DTYPE
        for name in ("q", "k", "v", "out", "cu", "lens") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
            assert _call(p, paged, kv8, cap=cap, **{name: None}) == AWQ_ERR_NULL, name
    for cap in (1e-30, 2.0, 3.4e38):                                 # every finite positive float is a cap
        assert _call(p, paged, kv8, cap=cap, cu=p + 2) == AWQ_ERR_ALIGN, cap
    # the order of the phases: null before dtype before shape (the cap's term in it) before alignment before the workspace
    assert _call(p, paged, kv8, cu=None, dtype=2, cap=NAN) == AWQ_ERR_NULL and _call(p, paged, kv8, dtype=2, cap=NAN, ws=None) == AWQ_ERR_DTYPE
    assert _call(p, paged, kv8, cap=NAN, cu=p + 2, ws=None) == AWQ_ERR_SHAPE and _call(p, paged, kv8, cu=p + 2, ws=None) == AWQ_ERR_ALIGN


def test_ops_attn_varq_softcap_refuses_a_bad_cap_before_any_work():
    q = torch.zeros(40, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    for extra in (dict(), dict(block_table=bt)):
        k = pool if extra else kc
        for bad in (-1.0, -INF, INF, NAN, 1e39):
            with pytest.raises(ValueError, match="softcap .* must be finite and not negative"):
                ops.attn_varq_softcap(q, k, k, cu, 30, lens, 256, bad, **extra)
        with pytest.raises(ValueError, match="softcap must be a float"):
            ops.attn_varq_softcap(q, k, k, cu, 30, lens, 256, None, **extra)
        with pytest.raises(ValueError, match="window_left -1 must not be negative"):
            ops.attn_varq_softcap(q, k, k, cu, 30, lens, 256, 50.0, -1, **extra)
        with pytest.raises(ValueError, match="window_left.*causal"):
            ops.attn_varq_softcap(q, k, k, cu, 30, lens, 256, 50.0, causal=False, **extra)
        for good in (dict(softcap=50.0), dict(softcap=0.0), dict(softcap=30, window_left=16)):
            with pytest.raises(RuntimeError, match="GPU"):          # a good cap gets as far as the GPU check, like a call without one
                ops.attn_varq_softcap(q, k, k, cu, 30, lens, 256, **good, **extra)


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
class _Attn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q_proj = self.k_proj = self.v_proj = self.o_proj = torch.nn.Identity()
        self.args = SimpleNamespace(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, rope_theta=10000.0, sliding_window=77,
                                    attn_logit_softcapping=50.0, query_pre_attn_scalar=144)
        self.kv_max_seq_len = 128


def test_make_quant_attn_softcap_passes_cap_scale_and_windows_through(monkeypatch):
    from llm_awq_amd import fused_attn

    seen = []
    monkeypatch.setattr(fused_attn, "fuse_qkv", lambda q, k, v: torch.nn.Identity())
    real = fused_attn.QuantLlamaAttentionFused

    def spy(*a, **kw):
        seen.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(fused_attn, "QuantLlamaAttentionFused", spy)
    monkeypatch.setattr(fused_attn, "isinstance", lambda o, c: False if c is spy else isinstance(o, c), raising=False)
    layers = lambda n: torch.nn.Sequential(*[_Attn() for _ in range(n)])
    out = fused_attn.make_quant_attn_softcap(layers(4), "cpu", 50.0, 144 ** -0.5, [33, None] * 2, max_batch_size=2)
    assert [m.sliding_window for m in out] == [33, None, 33, None] and [kw["sliding_window"] for kw in seen[-4:]] == [33, None, 33, None]
    assert all(m.attn_softcap == 50.0 and m.softmax_scale == 144 ** -0.5 for m in out)
    assert all(kw["attn_softcap"] == 50.0 and kw["softmax_scale"] == 144 ** -0.5 and kw["kv_layout"] == "natural" for kw in seen[-4:])
    out = fused_attn.make_quant_attn_softcap(layers(2), "cpu", 30.0, sliding_window=16)          # one window for every layer; Grok-1's cap
    assert [(m.sliding_window, m.attn_softcap, m.softmax_scale) for m in out] == [(16, 30.0, 64 ** -0.5)] * 2
    out = fused_attn.make_quant_attn_softcap(layers(2), "cpu", 30.0)                             # every layer global
    assert [(m.sliding_window, m.attn_softcap) for m in out] == [(None, 30.0)] * 2
    out = fused_attn.make_quant_attn(layers(1), "cpu", kv_layout="natural")                      # the config's values are never read
    assert out[0].attn_softcap is None and out[0].softmax_scale == 64 ** -0.5 and "attn_softcap" not in seen[-1]
    with pytest.raises(ValueError, match="3 entries for 2 attention modules"):
        fused_attn.make_quant_attn_softcap(layers(2), "cpu", 50.0, sliding_window=[4, None, 4])
    with pytest.raises(ValueError, match="attn_softcap"):
        fused_attn.make_quant_attn_softcap(layers(1), "cpu", None)
    for bad in (0.0, -1.0, INF, NAN, True, "50"):
        with pytest.raises(ValueError, match="attn_softcap"):
            fused_attn.make_quant_attn_softcap(layers(1), "cpu", bad)


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


def _module(monkeypatch, kv_dtype=None, kv_layout="natural", **kw):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0, sliding_window=77,
                           attn_logit_softcapping=50.0, query_pre_attn_scalar=144)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3,
                                            kv_layout=kv_layout, kv_dtype=kv_dtype, **kw)
    return m, spy


@pytest.mark.parametrize("window", [None, 33], ids=["global", "local"])
@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_routes_every_packed_call_to_the_softcap_entries(kv_dtype, paged, window, monkeypatch):
    scale = 144 ** -0.5
    m, spy = _module(monkeypatch, kv_dtype, sliding_window=window, attn_softcap=50.0, softmax_scale=scale)
    assert m.attn_softcap == 50.0 and m.softmax_scale == scale and m.sliding_window == window
    table = torch.zeros(3, 2, dtype=torch.int32)
    kw = dict(block_table=table, page_size=64) if paged else {}
    left = 127 if window is None else window - 1                      # a global layer: bound - 1 = 128 - 1, a window that hides nothing
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    name = "attn" + ("_paged" if paged else "") + "_varq_softcap" + ("_kv8" if kv_dtype else "")
    i = 1 + (4 if kv_dtype else 2) + paged
    out = m.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=2, split_min_keys=64, **kw)
    assert out.shape == (1, 140, 512) and [c[0] for c in spy.calls][1] == name and len(spy.calls) == 2
    aa = spy.calls[1][1]
    assert len(aa) == i + 11 and aa[i] is cu and aa[i + 1] == 96 and aa[i + 2] is pos and aa[i + 3] == 128
    # the thresholds, window_left, the cap, lens_before_step, the module's scale, causal
    assert aa[i + 4:] == (2, 64, left, 50.0, True, scale, True)
    spy.calls.clear()
    m.forward_packed(x, pos, freqs, cu, 96, **kw)                       # forward_packed is split_seqlen_q = 0
    assert spy.calls[1][0] == name and spy.calls[1][1][i + 4:] == (0, ops.ATTN_SPLIT_MIN_KEYS, left, 50.0, True, scale, True)
    spy.calls.clear()
    xr = torch.zeros(3, 2, 768, dtype=torch.float16)                    # forward under a tensor start_pos: the uniform cu, the packed route
    out = m(xr, pos, freqs, **kw)
    assert out.shape == (3, 2, 512) and spy.calls[1][0] == name
    aa = spy.calls[1][1]
    assert aa[0].shape == (6, 8, 64) and aa[i].tolist() == [0, 2, 4, 6] and aa[i].dtype == torch.int32 and aa[i + 1] == 2 and aa[i + 2] is pos
    assert aa[i + 4:] == (2, ops.ATTN_SPLIT_MIN_KEYS, left, 50.0, True, scale, True)
    if window is None and not paged:                                    # decode_max_seqlen is the bound a global layer's window follows
        spy.calls.clear()
        m.forward_packed(x, pos, freqs, cu, 96, decode_max_seqlen=100)
        assert spy.calls[1][1][i + 3] == 100 and spy.calls[1][1][i + 6] == 99


def test_softmax_scale_alone_reaches_every_path_that_takes_a_scale(monkeypatch):
    from llm_awq_amd import flash_attn_compat

    scale = 144 ** -0.5
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    m, spy = _module(monkeypatch, softmax_scale=scale)
    m.forward_packed(x, pos, freqs, cu, 96)
    m.forward_packed_split(x, pos, freqs, cu, 96)
    m(torch.zeros(3, 1, 768, dtype=torch.float16), pos, freqs)
    m(torch.zeros(3, 40, 768, dtype=torch.float16), pos, freqs)
    names = [c[0] for c in spy.calls]
    assert names[1::2] == ["attn_prefill_varq", "attn_varq", "attn_kvcache", "attn_prefill_kvcache"]       # the entries of a module without it
    assert [c[1][-2] for c in spy.calls[1::2]] == [scale] * 4
    got = {}
    monkeypatch.setattr(flash_attn_compat, "flash_attn_func", lambda q, k, v, **kw: got.update(kw) or torch.zeros_like(q))
    m(torch.zeros(3, 4, 768, dtype=torch.float16), 0, freqs)            # the host-length path of the natural layout
    assert got == dict(softmax_scale=scale, causal=True)
    ft, spy_ft = _module(monkeypatch, kv_layout="ft", softmax_scale=scale)
    ft(torch.zeros(3, 4, 768, dtype=torch.float16), 0, freqs)
    assert spy_ft.calls[1][0] == "attn_prefill_ftcache" and spy_ft.calls[1][1][5] == scale
    with pytest.raises(NotImplementedError, match="softmax_scale.*FT decode"):
        ft(torch.zeros(3, 1, 768, dtype=torch.float16), 4, freqs)


def test_module_without_the_keywords_calls_what_it_calls_today(monkeypatch):
    from llm_awq_amd import flash_attn_compat

    m, spy = _module(monkeypatch)                                       # the config's cap and scalar are there and are not read
    assert m.attn_softcap is None and m.softmax_scale == 64 ** -0.5
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    m.forward_packed(x, pos, freqs, cu, 96)
    m.forward_packed_split(x, pos, freqs, cu, 96)
    m(torch.zeros(3, 1, 768, dtype=torch.float16), pos, freqs)
    assert [c[0] for c in spy.calls] == ["rope_kv_store_natural_varq", "attn_prefill_varq", "rope_kv_store_natural_varq", "attn_varq",
                                         "rope_kv_store_natural_pos", "attn_kvcache"]
    assert [c[1][-2] for c in spy.calls[1::2]] == [64 ** -0.5] * 3
    w, spy_w = _module(monkeypatch, sliding_window=33)
    w.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=2, split_min_keys=64)
    assert spy_w.calls[1][0] == "attn_varq_window" and spy_w.calls[1][1][7:] == (2, 64, 32, True, 64 ** -0.5, True)
    got = {}
    monkeypatch.setattr(flash_attn_compat, "flash_attn_func", lambda q, k, v, **kw: got.update(kw) or torch.zeros_like(q))
    m(torch.zeros(3, 4, 768, dtype=torch.float16), 0, freqs)
    assert got == dict(causal=True)                                     # no softmax_scale keyword: the call of today
    ft, spy_ft = _module(monkeypatch, kv_layout="ft")
    ft(torch.zeros(3, 1, 768, dtype=torch.float16), 4, freqs)
    assert spy_ft.calls[-1][0] == "single_query_attention"


def test_module_refuses_what_the_cap_is_not_built_for_before_any_work(monkeypatch):
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    x = torch.zeros(3, 4, 768, dtype=torch.float16)
    m, spy = _module(monkeypatch, attn_softcap=50.0)
    with pytest.raises(NotImplementedError, match="attn_softcap.*int start_pos"):
        m(x, 0, freqs)
    with pytest.raises(NotImplementedError, match="attn_softcap.*int start_pos"):
        m(x[:, :1], 5, freqs)
    with pytest.raises(NotImplementedError, match="forward_shared.*attn_softcap"):
        m.forward_shared(x, pos, freqs, torch.zeros(3, 2, dtype=torch.int32), 64, None)
    ft, spy_ft = _module(monkeypatch, kv_layout="ft", attn_softcap=50.0)
    with pytest.raises(NotImplementedError, match="attn_softcap.*FT cache"):
        ft(x, 0, freqs)
    with pytest.raises(NotImplementedError, match="attn_softcap.*FT cache"):
        ft(x, pos, freqs)
    with pytest.raises(NotImplementedError, match="attn_softcap.*chunk_prefilling"):
        ft(x, 4, freqs, chunk_prefilling=True)
    with pytest.raises(NotImplementedError, match="attn_softcap.*FT cache"):
        ft.forward_packed(x.reshape(1, 12, 768), pos, freqs, torch.tensor([0, 4, 8, 12], dtype=torch.int32), 4)
    for name in ("attn_softcap", "softmax_scale"):
        for bad in (0, 0.0, -1.0, INF, NAN, True, "50"):
            with pytest.raises(ValueError, match=name):
                _module(monkeypatch, **{name: bad})
    assert not spy.calls and not spy_ft.calls
