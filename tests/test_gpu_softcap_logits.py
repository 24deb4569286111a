"""Final-logit soft-capping on the GPU (awq_logit_softcap, awq_lm_head_softcap, awq_lm_head_logprobs_softcap; csrc/awq_softcap.hpp):

    1. ops.logit_softcap_ against the float64 oracle within C * 2^-24 * cap (+ ulp_T / 2 for bf16 / fp16), inactive rows untouched
    2. ops.lm_head_softcap(out fp32) EQUALS logit_softcap_(ops.lm_head(..)) bit for bit -- the same device function on the same fp32 sums --
       and with out = T that value rounded once
    3. ops.lm_head_logprobs(softcap=c) on lattice rows: lse / logprob within tests/lm_logprobs_oracle.py's bounds on the capped logits,
       target_logit and argmax equal; edge targets, ignored rows
    4. softcap = 0 returns the bits of the uncapped entries
    5. LMHead(final_softcap=30) end to end on a synthetic head"""
import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from llm_awq_amd.lm_head import LMHead
from tests import lm_head_oracle as H
from tests import lm_logprobs_oracle as L
from tests import softcap_logits_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("logprob", "lse", "target_logit", "argmax")
VT = ops.lm_head_logprobs_plan(1, 1, 8)["vocab_tile"]          # host only
TORCH_T = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------------
# 1. logits that already exist
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
def test_logit_softcap_is_the_oracle_within_the_bound(dtype_name):
    for B, V in ((1, 1), (5, 1025), (64, 513)):       # one case a dtype: the shapes and the caps inside it
        for cap in (2.0, 30.0):
            _logit_softcap_is_the_oracle_within_the_bound(dtype_name, B, V, cap)


def _logit_softcap_is_the_oracle_within_the_bound(dtype_name, B, V, cap):
    T = TORCH_T[dtype_name]
    g = torch.Generator().manual_seed(1000 * B + V + int(cap))
    z = (torch.randn(B, V + 7, generator=g) * cap * 1.5).to(T)                  # |z| beyond 2 cap; a row stride wider than V
    special = torch.tensor([0.0, -0.0, 1e-30, cap, -cap, 2 * cap, -3 * cap, 1e4 * cap, -1e4 * cap, float("inf"), float("-inf")]).to(T)
    flat = z[:, :V].reshape(-1)
    n = min(flat.numel(), special.numel())
    z[:, :V] = torch.cat([special[:n], flat[n:]]).reshape(B, V)
    want_in = z.clone()
    zd = z.to(DEV)
    view = zd[:, :V]
    seqlens = None
    if B > 1:
        seqlens = torch.arange(1, B + 1, dtype=torch.int32)
        seqlens[[0, B // 2, B - 1]] = -1                                       # the first, a middle and the last row are inactive
        zd[0, 0] = float("nan")                                                # ... whatever they hold
    got = ops.logit_softcap_(view, cap, None if seqlens is None else seqlens.to(DEV))
    assert got.data_ptr() == view.data_ptr()
    out = zd.cpu()
    assert torch.equal(bits(out[:, V:]), bits(want_in[:, V:]))                 # nothing behind the row's V columns is touched
    active = np.ones(B, bool) if seqlens is None else seqlens.numpy() >= 0
    if B > 1:
        want_in[0, 0] = float("nan")
    assert torch.equal(bits(out[~torch.from_numpy(active)]), bits(want_in[~torch.from_numpy(active)]))
    z64 = H.f64(want_in[:, :V])[active]
    y = O.cap_f64(z64, cap)
    out_kind = "f32" if dtype_name == "fp32" else "T"
    bnd = O.bound(y, cap, 0.0, out_kind, "bf16" if dtype_name == "fp32" else dtype_name)
    err = np.abs(H.f64(out[:, :V])[active] - y)
    print(f"{dtype_name} B {B} V {V} cap {cap}: worst |err| / bound = {float((err / bnd).max()):.3f}")
    assert (err <= bnd).all(), (B, V, cap)
    nan = torch.full((1, 8), float("nan"), dtype=T, device=DEV)                # a NaN stays a NaN
    assert torch.isnan(ops.logit_softcap_(nan, cap)).all()


# ------------------------------------------------------------------------------------------------------------------------
# 2. the LM head's epilogue
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.NORM_SHAPES + [(1, 1025, 72), (64, 17, 8)], ids=lambda s: "m%d-v%d-k%d" % s)
def test_lm_head_softcap_equals_the_cap_of_the_lm_heads_logits_bit_for_bit(shape):
    for dtype_name in ("bf16", "fp16"):               # one case a shape: dtype, bias and norm inside it
        for with_bias in (False, True):
            for norm in (False, True):
                _lm_head_softcap_equals_the_cap_of_the_lm_heads_logits(shape, dtype_name, with_bias, norm)


def _lm_head_softcap_equals_the_cap_of_the_lm_heads_logits(shape, dtype_name, with_bias, norm):
    form = (dtype_name, with_bias, norm)
    M, V, K = shape
    c = H.build_norm_lattice(M, V, K, dtype_name, 1e-6)
    T = TORCH_T[dtype_name]
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    gamma = c["gamma"].to(DEV) if norm else None
    bias = (torch.randn(V, generator=torch.Generator().manual_seed(V)) * 0.5).to(T).to(DEV) if with_bias else None
    seqlens = torch.arange(1, M + 1, dtype=torch.int32, device=DEV)
    if M > 1:
        seqlens[M // 2] = -1
    plain = ops.lm_head(x, w, gamma, 1e-6, bias, seqlens)
    zmax = float(plain.abs().max())
    for cap in (30.0, zmax / 2):                                               # Gemma-2's, and one the logits reach twice over
        want = ops.logit_softcap_(plain.clone(), cap, seqlens)
        got = ops.lm_head_softcap(x, w, cap, gamma, 1e-6, bias, seqlens)
        assert got.dtype == torch.float32 and torch.equal(bits(got), bits(want)), (form, cap)
        assert not torch.equal(bits(got), bits(plain)), (form, cap)
        got_T = ops.lm_head_softcap(x, w, cap, gamma, 1e-6, bias, seqlens, out_dtype=T)
        assert got_T.dtype == T and torch.equal(bits(got_T), bits(want.to(T))), (form, cap)  # that value, rounded once
        if M > 1:
            assert not got[M // 2].any() and not got_T[M // 2].any()           # an inactive row of a fresh out: zeros
    eng = llm_awq_amd.load_engine()                                            # the engine binding gives the bits of ops
    assert torch.equal(bits(eng.lm_head_softcap(x, w, 30.0, gamma, 1e-6, bias, seqlens)), bits(ops.lm_head_softcap(x, w, 30.0, gamma, 1e-6, bias, seqlens))), form
    assert torch.equal(bits(eng.logit_softcap_(plain.clone(), 30.0, seqlens)), bits(ops.logit_softcap_(plain.clone(), 30.0, seqlens))), form


# ------------------------------------------------------------------------------------------------------------------------
# 3. the fused log-probabilities
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 17, 8), (129, 145, 72), (261, 273, 136)], ids=lambda s: "t%d-v%d-k%d" % s)
def test_lm_head_logprobs_softcap_is_within_the_bounds_on_the_capped_logits(shape):
    for dtype_name in ("bf16", "fp16"):               # one case a shape: dtype, bias and round_logits inside it
        for with_bias in (False, True):
            for round_logits in (False, True):
                _lm_head_logprobs_softcap_is_within_the_bounds(shape, dtype_name, with_bias, round_logits)


def _lm_head_logprobs_softcap_is_within_the_bounds(shape, dtype_name, with_bias, round_logits):
    form = (dtype_name, with_bias, round_logits)
    Tn, V, K = shape
    case = L.build_lattice(Tn, V, K, dtype_name, with_bias, VT)
    T = TORCH_T[dtype_name]
    z = L.case_reference(case, round_logits, targets=None)["z"]               # exact on the lattice (rounded to T under round_logits)
    cap = float(np.abs(z).max()) / 2
    zt = torch.from_numpy(z).to(T if round_logits else torch.float32)
    assert np.array_equal(H.f64(zt), z)
    capped = H.f64(ops.logit_softcap_(zt.to(DEV), cap))                        # test 1's function: fp32, or T rounded once more
    ignored = L.ignored_patterns(Tn, V) if Tn > 1 else []
    targets = L.edge_targets(Tn, V, VT, ignored)
    fill = -7.0
    init = {n: np.full(Tn, fill) for n in ALL}
    want = L.from_logits(capped, targets, init)
    bnd = L.bounds(capped, targets, 0.0, -(-V // VT))
    x = _dev(case["x3"])[:, 2, :]
    out = {n: torch.full((Tn,), fill, dtype=torch.int32 if n == "argmax" else torch.float32, device=DEV) for n in ALL}
    res = ops.lm_head_logprobs(x, _dev(case["w"]), _dev(targets), bias=_dev(case["bias"]), round_logits=round_logits, want=ALL, out=out, softcap=cap)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert not L.mismatches(got, want, bnd), form
    assert np.array_equal(got["argmax"], want["argmax"]) and np.array_equal(got["target_logit"].astype(np.float64), want["target_logit"]), form
    plain = ops.lm_head_logprobs(x, _dev(case["w"]), _dev(targets), bias=_dev(case["bias"]), round_logits=round_logits, want=ALL)
    if Tn > 1:
        assert not np.array_equal(plain["lse"].cpu().numpy(), got["lse"]), form
    eng = llm_awq_amd.load_engine()
    e = eng.lm_head_logprobs_softcap(x, _dev(case["w"]), cap, _dev(targets), None, 0.0, _dev(case["bias"]), round_logits)
    act = torch.from_numpy(want["active"])
    for name, t in zip(ALL, e):
        assert torch.equal(t.cpu()[act], res[name].cpu()[act]), (form, name)


# ------------------------------------------------------------------------------------------------------------------------
# 4. no cap
# ------------------------------------------------------------------------------------------------------------------------
def test_softcap_0_returns_the_bits_of_the_uncapped_entries():
    c = H.build_norm_lattice(17, 65, 1032, "bf16", 1e-6)
    x, w, gamma = c["x"].to(DEV), c["w"].to(DEV), c["gamma"].to(DEV)
    for out_dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(bits(ops.lm_head_softcap(x, w, 0.0, gamma, 1e-6, out_dtype=out_dtype)), bits(ops.lm_head(x, w, gamma, 1e-6, out_dtype=out_dtype)))
    z = ops.lm_head(x, w, gamma, 1e-6)
    assert torch.equal(bits(ops.logit_softcap_(z.clone(), 0.0)), bits(z))
    tg = torch.arange(17, dtype=torch.int32, device=DEV)
    for rl in (False, True):
        a = ops.lm_head_logprobs(x, w, tg, gamma, 1e-6, round_logits=rl, want=ALL, softcap=0.0)
        b = ops.lm_head_logprobs(x, w, tg, gamma, 1e-6, round_logits=rl, want=ALL)
        assert all(torch.equal(a[n], b[n]) for n in ALL)
        capped = ops.lm_head_logprobs(x, w, tg, gamma, 1e-6, round_logits=rl, want=ALL, softcap=0.5)
        assert not torch.equal(capped["lse"], b["lse"])


# ------------------------------------------------------------------------------------------------------------------------
# 5. the module
# ------------------------------------------------------------------------------------------------------------------------
def test_lm_head_module_with_a_final_softcap_end_to_end():
    g = torch.Generator().manual_seed(9)
    K, V, B, S = 136, 1025, 5, 3
    w = torch.randn(V, K, generator=g).to(torch.bfloat16).to(DEV)              # logits of a few tens: the cap of 30 bites
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(DEV)
    h = torch.randn(B, S, K, generator=g).to(torch.bfloat16).to(DEV)
    head, plain = LMHead(w, gamma, 1e-6, final_softcap=30.0), LMHead(w, gamma, 1e-6)
    logits = head(h)
    assert torch.equal(bits(logits), bits(ops.logit_softcap_(plain(h), 30.0))) and float(plain(h).abs().max()) > 30.0 >= float(logits.abs().max())
    xn = H.f64(ops.rmsnorm(h[:, -1, :].contiguous(), gamma, 1e-6))
    z = xn @ H.f64(w).T
    y = O.cap_f64(z, 30.0)
    bnd = O.bound(y, 30.0, H.bound(np.abs(xn) @ np.abs(H.f64(w)).T, K))
    assert (np.abs(H.f64(logits) - y) <= bnd).all()
    tg = torch.randint(0, V, (B * S,), generator=g).to(torch.int32).to(DEV)
    res = head.logprobs(h, tg, want=ALL)
    ref = ops.lm_head_logprobs(h.reshape(-1, K), w, tg, gamma, 1e-6, want=ALL, softcap=30.0)
    assert all(torch.equal(res[n], ref[n]) for n in ALL)
    own = ops.token_logprobs(ops.logit_softcap_(ops.lm_head(h.reshape(-1, K), w, gamma, 1e-6), 30.0), tg)      # the unfused route, for the values
    assert torch.allclose(res["logprob"], own["logprob"], rtol=0, atol=1e-3) and torch.equal(res["argmax"], own["argmax"])
