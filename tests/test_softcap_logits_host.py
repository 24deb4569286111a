"""Final-logit soft-capping without a GPU: the float64 oracle and its bound, every mutant seen on lattice logits whose magnitude reaches
twice the cap, the exports and the signatures that must stay, and every refusal of the three C entries and of the ops wrappers before a launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import lm_head_oracle as H
from tests import lm_logprobs_oracle as L
from tests import softcap_logits_oracle as O

AWQ_OK, AWQ_ERR_BATCH, AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = 0, -1, -3, -4, -5, -6, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
BAD_CAPS = (-1.0, -1e-30, -INF, INF, NAN)
I, VP, SZ, F, LONG = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_long


# ------------------------------------------------------------------------------------------------------------------------
# the oracle, its bound and the mutants
# ------------------------------------------------------------------------------------------------------------------------
def test_oracle_by_hand_and_at_the_ends():
    for cap in (2.0, 30.0):
        z = np.array([0.0, cap * np.arctanh(0.5), -cap * np.arctanh(0.5), 1e30, -1e30, INF, -INF, NAN])
        y = O.cap_f64(z, cap)
        assert np.allclose(y[:3], [0.0, cap / 2, -cap / 2], rtol=1e-15, atol=0) and list(y[3:7]) == [cap, -cap, cap, -cap] and np.isnan(y[7])
        assert np.allclose(O.cap_f64(np.array([1e-3]), 1e12), 1e-3, rtol=1e-12)          # cap -> inf: the logit itself
    assert O.C <= 16 and O.bound(np.array([1.0]), 30.0)[0] == O.C * 2.0 ** -24 * 30.0
    b = O.bound(np.array([1.0]), 30.0, 0.25, "T", "bf16")[0]
    assert b == O.C * 2.0 ** -24 * 30.0 + 0.25 + 2.0 ** -8                                # ulp_bf16 in [1, 2) is 2^-7


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(16, 127, 1032), (64, 15, 72), (17, 1025, 8)], ids=lambda s: "m%d-v%d-k%d" % s)
def test_every_mutant_is_seen_on_logits_that_reach_twice_the_cap(shape, dtype_name):
    case = H.build_lattice(*shape, dtype_name, True)
    zmax = float(np.abs(case["y_f32"]).max())
    cap = zmax / 2                                                   # the lattice scaled against the cap: |z| reaches 2 cap
    assert cap > 0
    for out in ("f32", "T"):
        want, y, bnd = O.lm_head_case(case, cap, out)
        assert (np.abs(want - y) <= bnd).all()                       # the contract's own value lies inside its bound
        for mutant in O.MUTANTS:
            if mutant == "cap-after-round" and out == "f32":
                continue
            got = O.lm_head_case(case, cap, out, mutant)[0]
            seen = int((np.abs(got - y) > bnd).sum())
            print(f"{shape} {dtype_name} out {out} cap {cap:.4g} {mutant}: {seen} of {got.size} elements beyond the bound")
            assert seen > 0, (out, mutant)


@pytest.mark.parametrize("round_logits", [False, True], ids=["f32", "rounded"])
def test_mutants_are_seen_through_the_logprob_outputs(round_logits):
    """The same faults as the fused log-prob entry would show them: through lse / logprob / target_logit under tests/lm_logprobs_oracle.py's check."""
    vt = 128
    case = L.build_lattice(129, 145, 72, "bf16", True, vt)
    ref = L.case_reference(case, False)
    z, bias = ref["z"], H.f64(case["bias"])
    cap = float(np.abs(z).max()) / 2
    out = "T" if round_logits else "f32"
    pre = H.round_T(z, "bf16") if round_logits else z                # round_logits: rounded to T, capped, rounded once more
    truth = O.capped(pre, cap, bias, out, "bf16")
    want = L.from_logits(truth, case["targets"])
    bnd = L.bounds(truth, case["targets"], 0.0, -(-145 // vt))
    assert not L.mismatches({k: want[k] for k in ("logprob", "lse", "target_logit", "argmax")}, want, bnd)
    for mutant in ("nocap", "cap-before-bias"):
        got = L.from_logits(O.capped(pre, cap, bias, out, "bf16", mutant), case["targets"])
        assert L.mismatches(got, want, bnd), mutant
    if round_logits:                                                 # the second rounding left out
        got = L.from_logits(O.capped(pre, cap, bias, "f32", "bf16"), case["targets"])
        assert L.mismatches(got, want, bnd)


# ------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_the_signatures_that_stay():
    Lb = ctypes.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    S_ = _capi.SIGNATURES
    for name in ("awq_logit_softcap", "awq_lm_head_softcap", "awq_lm_head_logprobs_softcap"):
        assert hasattr(Lb, name) and name in S_ and re.search(r"\bint " + name + r"\(", header), name
    assert _capi.lib().awq_abi_version() == 1
    base = list(S_["awq_lm_head"][1])
    assert list(S_["awq_lm_head_softcap"][1]) == base[:-2] + [F] + base[-2:]                    # softcap in front of max_blocks
    base = list(S_["awq_lm_head_logprobs"][1])
    assert list(S_["awq_lm_head_logprobs_softcap"][1]) == base[:-4] + [F] + base[-4:]            # softcap behind round_logits
    assert list(S_["awq_logit_softcap"][1]) == [VP, I, LONG, VP, I, I, F, VP]
    # ops.lm_head and the first nine parameters of ops.lm_head_logprobs are as they were
    assert list(inspect.signature(ops.lm_head).parameters) == ["x", "weight", "gamma", "eps", "bias", "seqlens", "out", "out_dtype", "max_blocks"]
    lp = inspect.signature(ops.lm_head_logprobs).parameters
    assert list(lp)[:9] == ["x", "weight", "targets", "gamma", "eps", "bias", "round_logits", "ws", "want"]
    assert list(lp)[-1] == "softcap" and lp["softcap"].kind is inspect.Parameter.KEYWORD_ONLY and lp["softcap"].default == 0.0
    assert list(inspect.signature(ops.lm_head_softcap).parameters) == ["x", "weight", "softcap", "gamma", "eps", "bias", "seqlens", "out", "out_dtype",
                                                                       "max_blocks"]
    assert list(inspect.signature(ops.logit_softcap_).parameters) == ["logits", "softcap", "seqlens"]
    eng = llm_awq_amd.load_engine()
    for name in ("lm_head_softcap", "logit_softcap_", "lm_head_logprobs_softcap", "lm_head", "lm_head_logprobs", "token_logprobs"):
        assert hasattr(eng, name), name
    assert "softcap:" not in eng.lm_head.__doc__.splitlines()[0] and "weight: torch.Tensor, softcap:" in eng.lm_head_softcap.__doc__.splitlines()[0]
    from llm_awq_amd import evaluate
    from llm_awq_amd.lm_head import LMHead

    assert list(inspect.signature(LMHead.__init__).parameters)[-1] == "final_softcap"
    assert inspect.signature(LMHead.__init__).parameters["final_softcap"].default is None
    for fn in (evaluate.perplexity, evaluate.loglikelihood, evaluate.perplexity_hf):
        assert inspect.signature(fn).parameters["final_softcap"].default is None


# ------------------------------------------------------------------------------------------------------------------------
# refusals: no launch
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_logit_softcap_refuses_without_a_launch():
    buf, p = _p16()
    fn = _capi.lib().awq_logit_softcap
    ok = dict(logits=p, dt=_capi.AWQ_F32, ld=1025, lens=p, b=5, v=1025, cap=30.0)
    call = lambda **kw: fn(*[dict(ok, **kw)[k] for k in ("logits", "dt", "ld", "lens", "b", "v", "cap")], None)
    for bad in BAD_CAPS:
        assert call(cap=bad) == AWQ_ERR_SHAPE, bad
        assert call(cap=bad, logits=p + 1) == AWQ_ERR_SHAPE, bad      # the shape phase stands in front of the alignment
    assert call(logits=None) == AWQ_ERR_NULL and call(logits=None, cap=NAN, dt=7) == AWQ_ERR_NULL
    assert call(dt=3) == AWQ_ERR_DTYPE and call(dt=-1, cap=NAN) == AWQ_ERR_DTYPE
    for bad in (dict(b=0), dict(v=0), dict(ld=1024), dict(v=(1 << 30) + 1, ld=1 << 31)):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    assert call(logits=p + 2) == AWQ_ERR_ALIGN and call(logits=p + 1, dt=_capi.AWQ_BF16) == AWQ_ERR_ALIGN and call(lens=p + 2) == AWQ_ERR_ALIGN
    assert call(cap=0.0) == AWQ_OK and call(cap=0.0, lens=None) == AWQ_OK        # no cap: every check, then nothing is launched


def test_lm_head_softcap_refuses_without_a_launch():
    buf, p = _p16()
    fn = _capi.lib().awq_lm_head_softcap
    ok = dict(x=p, ldx=72, gamma=p, eps=1e-6, w=p, bias=p, lens=p, out=p, odt=_capi.AWQ_F32, m=5, v=130, k=72, dt=_capi.AWQ_BF16, cap=30.0, mb=0)
    keys = list(ok)
    call = lambda **kw: fn(*[dict(ok, **kw)[k] for k in keys], None)
    for cap in (30.0, 0.0):                                          # the sibling's codes, with a cap and as the sibling itself
        assert call(cap=cap, x=None) == AWQ_ERR_NULL and call(cap=cap, dt=2) == AWQ_ERR_DTYPE and call(cap=cap, odt=_capi.AWQ_F16) == AWQ_ERR_DTYPE
        assert call(cap=cap, m=0) == AWQ_ERR_BATCH and call(cap=cap, m=65) == AWQ_ERR_BATCH
        for bad in (dict(v=0), dict(k=12), dict(ldx=64), dict(ldx=76), dict(mb=-1)):
            assert call(cap=cap, **bad) == AWQ_ERR_SHAPE, bad
        assert call(cap=cap, w=p + 8) == AWQ_ERR_ALIGN and call(cap=cap, lens=p + 2) == AWQ_ERR_ALIGN
    for bad in BAD_CAPS:
        assert call(cap=bad) == AWQ_ERR_SHAPE and call(cap=bad, w=p + 8) == AWQ_ERR_SHAPE, bad
    assert call(cap=NAN, m=0) == AWQ_ERR_BATCH and call(cap=NAN, dt=2) == AWQ_ERR_DTYPE


def test_lm_head_logprobs_softcap_refuses_without_a_launch():
    buf, p = _p16()
    fn = _capi.lib().awq_lm_head_logprobs_softcap
    need = ops.lm_head_logprobs_workspace_bytes(129, 145, 72, True)
    ok = dict(x=p, ldx=72, gamma=p, eps=1e-6, w=p, bias=p, tg=p, lp=p, lse=p, tl=p, am=p, t=129, v=145, k=72, dt=_capi.AWQ_BF16, rl=1, cap=30.0,
              ws=p, wsb=1 << 40, mb=0)
    keys = list(ok)
    call = lambda **kw: fn(*[dict(ok, **kw)[k] for k in keys], None)
    for cap in (30.0, 0.0):
        assert call(cap=cap, x=None) == AWQ_ERR_NULL and call(cap=cap, tg=None) == AWQ_ERR_NULL and call(cap=cap, dt=2) == AWQ_ERR_DTYPE
        for bad in (dict(t=0), dict(v=0), dict(k=12), dict(ldx=64), dict(mb=-1), dict(ldx=80)):       # (with gamma, ldx must equal k)
            assert call(cap=cap, **bad) == AWQ_ERR_SHAPE, bad
        assert call(cap=cap, w=p + 8) == AWQ_ERR_ALIGN and call(cap=cap, lse=p + 2) == AWQ_ERR_ALIGN
        assert call(cap=cap, ws=None) == AWQ_ERR_WORKSPACE and call(cap=cap, wsb=need - 1) == AWQ_ERR_WORKSPACE
    for bad in BAD_CAPS:
        assert call(cap=bad) == AWQ_ERR_SHAPE and call(cap=bad, ws=None, w=p + 8) == AWQ_ERR_SHAPE, bad
    assert call(cap=NAN, dt=2) == AWQ_ERR_DTYPE and call(cap=NAN, x=None) == AWQ_ERR_NULL


def test_ops_wrappers_refuse_a_bad_cap_before_any_work():
    x, w = torch.zeros(3, 72, dtype=torch.bfloat16), torch.zeros(130, 72, dtype=torch.bfloat16)
    z = torch.zeros(3, 130)
    for bad in (-1.0, -INF, INF, NAN, 1e39):
        with pytest.raises(ValueError, match="lm_head_softcap: softcap .* must be finite and not negative"):
            ops.lm_head_softcap(x, w, bad)
        with pytest.raises(ValueError, match="lm_head_logprobs: softcap .* must be finite and not negative"):
            ops.lm_head_logprobs(x, w, softcap=bad)
    with pytest.raises(ValueError, match="softcap must be a float"):
        ops.lm_head_softcap(x, w, None)
    with pytest.raises(TypeError):
        ops.lm_head_logprobs(x, w, None, None, 0.0, None, False, None, ("lse",), None, 0, 30.0)      # keyword-only
    for cap in (30.0, 0.0):                                          # a good cap gets as far as the GPU check
        with pytest.raises(RuntimeError, match="GPU"):
            ops.lm_head_softcap(x, w, cap)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.lm_head_logprobs(x, w, softcap=cap)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.logit_softcap_(z, 30.0)
    from llm_awq_amd.lm_head import LMHead

    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="final_softcap"):
            LMHead(w, final_softcap=bad)
    assert LMHead(w).final_softcap is None and LMHead(w, final_softcap=30).final_softcap == 30.0


def test_head_and_evaluate_hand_the_cap_through(monkeypatch):
    from llm_awq_amd import evaluate, lm_head

    calls = []
    monkeypatch.setattr(lm_head.ops, "lm_head", lambda *a, **kw: calls.append(("lm_head", a, kw)))
    monkeypatch.setattr(lm_head.ops, "lm_head_softcap", lambda *a, **kw: calls.append(("lm_head_softcap", a, kw)))
    monkeypatch.setattr(lm_head.ops, "lm_head_logprobs", lambda *a, **kw: calls.append(("lm_head_logprobs", a, kw)) or
                        {"logprob": torch.zeros(a[0].shape[0]), "argmax": torch.zeros(a[0].shape[0], dtype=torch.int32)})
    w = torch.zeros(130, 72, dtype=torch.bfloat16)
    h = torch.zeros(4, 72, dtype=torch.bfloat16)
    tg = torch.zeros(4, dtype=torch.int32)
    plain, capped = lm_head.LMHead(w), lm_head.LMHead(w, final_softcap=30.0)
    plain(h), plain.logprobs(h, tg)
    assert [c[0] for c in calls] == ["lm_head", "lm_head_logprobs"] and calls[1][2] == {} and len(calls[1][1]) == 10     # the calls of today
    calls.clear()
    capped(h), capped.logprobs(h, tg), plain.logprobs(h, tg, final_softcap=2.0)
    assert calls[0][0] == "lm_head_softcap" and calls[0][1][2] == 30.0 and calls[0][1][1] is w
    assert calls[1][2] == {"softcap": 30.0} and calls[2][2] == {"softcap": 2.0}
    calls.clear()
    ids = torch.arange(16) % 7
    evaluate.perplexity(lambda b: torch.zeros(b.shape[1], 72, dtype=torch.bfloat16), plain, ids, seqlen=8, final_softcap=30.0)
    evaluate.loglikelihood(lambda b: torch.zeros(b.shape[1], 72, dtype=torch.bfloat16), plain, ids[:5], ids[5:8], final_softcap=30.0)
    assert len(calls) == 3 and all(c[2] == {"softcap": 30.0} for c in calls)
    calls.clear()
    evaluate.perplexity(lambda b: torch.zeros(b.shape[1], 72, dtype=torch.bfloat16), plain, ids, seqlen=8)
    assert all(c[2] == {} for c in calls)

    class Model:
        lm_head = torch.nn.Linear(72, 130, bias=False).to(torch.bfloat16)
        model = staticmethod(lambda b: (torch.zeros(b.shape[1], 72, dtype=torch.bfloat16),))
    calls.clear()
    evaluate.perplexity_hf(Model, ids, seqlen=8, final_softcap=30.0)
    assert len(calls) == 2 and all(c[2] == {"softcap": 30.0} for c in calls)
