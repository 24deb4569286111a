"""Restatements of the reference's W8A8 family (awq/kernels/csrc/w8a8/) in integer, float64 and IEEE float32 arithmetic on the CPU.

GEMM (w8a8_gemm_cuda.cu): acc = x_i8 . w_i8^T in int32 (mma.sync s8, exact); epilogue in fp32
    with bias  (:575-578)  psums = float(acc) * wscale * ascale + bias        (one fused multiply-add for the last two steps)
    no bias    (:896-898)  psums = float(acc) * (wscale * ascale)
    out = __float22half2_rn(psums).
invoke_quant (quantization.cu:56-92): amax = max |float(x)|, scale = half_rn(amax / 127), q = float_to_int8_rn(float(x) * (127 / amax))
    (cvt.rni.sat.s8.f32: nearest-even, saturating, NaN -> 0).
gelu_and_quant (act.cu:22-77): gelu_fast with every step rounded to fp16 (:23-28), tmp = g, amax over (g > 0.0001h ? g : -g) from 0,
    scale = half(amax / 127), q = float_to_int8_rn(half(127 / amax) * g) with that product in fp16.
rms_norm_general (layernorm.cu:55-188, :193-232): LayerNorm with mean subtraction; per token amax = max(max |T(v)|, T(1e-6)),
    q = int8(v * (127 / amax)), scale = amax / 127; per tensor q = int8(v * scaling[0]) with beta not applied.

Everything here runs on CPU tensors: torch's CPU float32 add / mul / div are IEEE operations with one rounding.

Every restatement takes `mutant=`: one name switches one plausible fault in, for the host tests (tests/test_w8a8_host.py) that prove
the GPU checks of tests/w8a8_cases.py can see it.
    GEMM_MUTANTS   assoc           no bias: (float(acc) * ws) * as, two roundings instead of one (ws * as is exact in fp32)
                   nofma           bias: the product t * as rounded before the addition
                   assoc_bias      bias: fmaf(float(acc), ws * as, bias)
                   exact           the exact value of acc ws as + bias rounded to fp32 once (acc itself not rounded to a float first)
                   trunc           int -> float conversion toward zero (seen only where |acc| > 2^24)
                   bias_first      (float(acc) * ws + bias) * as
                   droptail        the last K % 64 columns not summed (in acc_exact)
    QUANT_MUTANTS  half_away       ties away from zero in the int8 conversion
                   inv_from_scale  1 / float(half(amax / 127)) instead of 127 / amax
                   trunc           truncation instead of rounding
    GELU_MUTANTS   single_rounding GELU evaluated in high precision and rounded to fp16 once
                   plain_abs       amax over |g|, without the 1e-4 quirk
                   prod_f32        inv * g not rounded to fp16 before the conversion
                   inv_f32         127 / amax not rounded to fp16
    LN_MUTANTS     noeps, eps_outside (1 / (sqrt(var) + eps)), rms (no mean subtraction), unbiased (K - 1), amax_unrounded (amax over v
                   instead of T(v)), scale_row (per tensor reads scaling[row]), beta_tensor (beta applied per tensor), nobeta_token
                   (beta ignored per token), scale_divides (per tensor q = v / scaling[0])
Dropping the T(1e-6) floor of the per-token amax is NOT a mutant.  For a row whose v is all zero it cannot be observed: 127 / 0 = inf and
0 * inf = NaN -> q = 0, the same q as with the floor, and the scale 1e-6 / 127 rounds to 0 in fp16, the same as 0 / 127.  Any other row has
max |n| >= 1, so only a |gamma| below 1e-6 could bring max |T(v)| under the floor; no test is invented for that.
"""
from __future__ import annotations

import torch

GEMM_MUTANTS = ("assoc", "nofma", "assoc_bias", "exact", "trunc", "bias_first", "droptail")
QUANT_MUTANTS = ("half_away", "inv_from_scale", "trunc")
GELU_MUTANTS = ("single_rounding", "plain_abs", "prod_f32", "inv_f32")
LN_MUTANTS = ("noeps", "eps_outside", "rms", "unbiased", "amax_unrounded", "scale_row", "beta_tensor", "nobeta_token", "scale_divides")


def _known(mutant, names):
    if mutant is not None and mutant not in names:
        raise ValueError(mutant)


def acc_exact(x_i8: torch.Tensor, w_i8: torch.Tensor, mutant=None) -> torch.Tensor:
    """x [M, K] . w [N, K]^T as int64; computed in float64, exact since |acc| <= K * 2^14 < 2^53."""
    _known(mutant, GEMM_MUTANTS)
    k = x_i8.shape[1]
    if mutant == "droptail":
        k -= k % 64
    return (x_i8.cpu()[:, :k].double() @ w_i8.cpu()[:, :k].double().t()).round().long()


def gemm_f64(acc: torch.Tensor, wscales, ascales, bias=None):
    """-> (e float64 [M, N], mag = |acc ws as| + |bias|)."""
    p = acc.double() * wscales.cpu().double()[None, :] * ascales.cpu().double()[:, None]
    b = torch.zeros_like(p) if bias is None else bias.cpu().double()[None, :].expand_as(p)
    return p + b, p.abs() + b.abs()


def _add_f32(p: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """float32(p + c) with ONE rounding, p and c float64: the float64 sum is made round-to-odd with the error term of TwoSum, after
    which the rounding to 24 bits is the rounding of the exact sum (53 >= 24 + 2)."""
    p, c = (t.contiguous() for t in torch.broadcast_tensors(p, c))
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # s + e == p + c exactly
    even = (s.view(torch.int64) & 1) == 0
    away = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where((e != 0) & even, torch.nextafter(s, away), s).to(torch.float32)


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf on float32 values: the product of two float32 is exact in float64."""
    return _add_f32(a.double() * b.double(), c.double())


def gemm_f32(acc: torch.Tensor, wscales, ascales, bias=None, mutant=None) -> torch.Tensor:
    """The specified fp32 epilogue, step by step (float32 [M, N], not yet rounded to fp16)."""
    _known(mutant, GEMM_MUTANTS)
    a32 = acc.to(torch.float32)  # int -> float32, nearest-even
    if mutant == "trunc":
        a32 = torch.where(a32.double().abs() > acc.double().abs(), torch.nextafter(a32, torch.zeros_like(a32)), a32)
    ws, as_ = wscales.cpu().float()[None, :], ascales.cpu().float()[:, None]
    b = None if bias is None else bias.cpu().float()[None, :]
    if mutant == "exact":  # acc (< 2^27) times ws as (22 bits) is exact in float64
        p = acc.double() * (ws.double() * as_.double())
        return _add_f32(p, torch.zeros_like(p) if b is None else b.double())
    if mutant == "bias_first":
        return (a32 * ws + (0.0 if b is None else b)) * as_
    if b is None:
        return (a32 * ws) * as_ if mutant == "assoc" else a32 * (ws * as_)
    if mutant == "assoc_bias":
        return _fma32(a32, ws * as_, b)
    t = a32 * ws
    if mutant == "nofma":
        return t * as_ + b
    return _fma32(t, as_, b)


def sat_s8(y: torch.Tensor, mutant=None) -> torch.Tensor:
    """float_to_int8_rn: nearest-even, saturating, NaN -> 0."""
    _known(mutant, QUANT_MUTANTS)
    y = torch.where(torch.isnan(y), torch.zeros_like(y), y)
    if mutant == "half_away":
        r = torch.sign(y) * torch.floor(y.abs() + 0.5)
    elif mutant == "trunc":
        r = torch.trunc(y)
    else:
        r = torch.round(y)
    return r.clamp_(-128, 127).to(torch.int8)


def quant_per_token(x: torch.Tensor, mutant=None):
    """x T [.., K] -> (q int8 [tokens, K], scale fp16 [tokens]) in IEEE float32."""
    _known(mutant, QUANT_MUTANTS)
    xf = x.cpu().float().reshape(-1, x.shape[-1])
    amax = xf.abs().amax(-1)
    scale = (amax / 127.0).to(torch.float16)
    if mutant == "inv_from_scale":
        inv = (torch.ones_like(amax) / scale.float())[:, None]
    else:
        inv = (torch.full_like(amax, 127.0) / amax)[:, None]  # inf for an all-zero row: 0 * inf = NaN -> 0
    return sat_s8(xf * inv, mutant), scale


_H = torch.float16


def _hmul(a, b):
    return (a.float() * b.float()).to(_H)  # the product of two fp16 values is exact in float32: one rounding


def _hadd(a, b):
    return (a.double() + b.double()).to(torch.float32).to(_H)  # the sums used here are exact in float32 or far from an fp16 tie


def gelu_fast_steps(x: torch.Tensor):
    """x fp16 -> (u = a * e in fp16, hx = 0.5h * x): g = hx * (1h + half(tanhf(float(u))))."""
    x = x.cpu()
    one = torch.tensor(1.0, dtype=_H)
    a = _hmul(x, torch.tensor(0.79788456, dtype=torch.float32).to(_H))
    c = _hmul(torch.tensor(0.044715, dtype=torch.float32).to(_H), x)
    e = _hadd(one, _hmul(c, x))
    return _hmul(a, e), _hmul(torch.tensor(0.5, dtype=_H), x)


def gelu_from_tanh(hx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    return _hmul(hx, _hadd(torch.tensor(1.0, dtype=_H), t))


def gelu_candidates(x: torch.Tensor, delta: float, mutant=None):
    """-> (g_lo, g_hi) fp16: gelu_fast(x) with tanh rounded to fp16 from tanh(u) (1 - delta) and tanh(u) (1 + delta).  Where the two
    agree the rounding of tanh is decided and so is g; where they differ, either neighbour is a correct result."""
    _known(mutant, GELU_MUTANTS)
    if mutant == "single_rounding":
        xd = x.cpu().double()
        g = (0.5 * xd * (1.0 + torch.tanh(0.79788456 * xd * (1.0 + 0.044715 * xd * xd)))).to(torch.float32).to(_H)
        return g, g
    u, hx = gelu_fast_steps(x)
    th = torch.tanh(u.double())
    t_lo, t_hi = (th * (1.0 - delta)).to(torch.float32).to(_H), (th * (1.0 + delta)).to(torch.float32).to(_H)
    return gelu_from_tanh(hx, t_lo), gelu_from_tanh(hx, t_hi)


def gelu_quant_from_tmp(g: torch.Tensor, mutant=None):
    """g fp16 [.., K] (the kernel's tmp) -> (q int8 [tokens, K], scale fp16 [tokens]); the quantisation stage of act.cu:45-68."""
    _known(mutant, GELU_MUTANTS)
    g = g.cpu().reshape(-1, g.shape[-1])
    t = (g.abs() if mutant == "plain_abs" else torch.where(g > torch.tensor(0.0001, dtype=torch.float32).to(_H), g, -g)).float()
    amax = t.amax(-1).clamp_min(0.0) + 0.0  # amax_val starts at +0 (and -0 + 0 = +0: the sign of 127 / amax matters when amax is 0)
    scale = (amax / 127.0).to(_H)
    inv = (torch.full_like(amax, 127.0) / amax)[:, None]
    if mutant == "inv_f32":
        return sat_s8((inv * g.float()).to(_H).float()), scale
    inv = inv.to(_H)
    if mutant == "prod_f32":
        return sat_s8(inv.float() * g.float()), scale
    return sat_s8(_hmul(inv.expand_as(g), g).float()), scale


def layernorm_quant_f64(x, gamma, beta, eps: float, per_token: bool, scaling=None, mutant=None):
    """-> (y64 [tokens, K]: the unrounded value whose nearest integer is q, amax64 [tokens] or None, mag = |n gamma| + |beta| [tokens, K]).
    n = (x - mean) rsqrt(var + eps) in float64; amax is taken over v rounded to x's dtype (layernorm.cu:146-150)."""
    _known(mutant, LN_MUTANTS)
    T = x.dtype
    xd = x.cpu().double().reshape(-1, x.shape[-1])
    K = xd.shape[-1]
    mean = torch.zeros(xd.shape[0], 1, dtype=torch.float64) if mutant == "rms" else xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / (K - 1 if mutant == "unbiased" else K)
    if mutant == "noeps":
        den = torch.sqrt(var)
    elif mutant == "eps_outside":
        den = torch.sqrt(var) + eps
    else:
        den = torch.sqrt(var + eps)
    ng = (xd - mean) / den * gamma.cpu().double()[None, :]
    b = torch.zeros_like(ng) if beta is None else beta.cpu().double()[None, :].expand_as(ng)
    if not per_token:
        s = scaling.cpu().double()
        mul = s[:xd.shape[0], None] if mutant == "scale_row" else s[0]
        v = ng + b if mutant == "beta_tensor" else ng
        return (v / mul if mutant == "scale_divides" else v * mul), None, ng.abs()
    if mutant == "nobeta_token":
        b = torch.zeros_like(ng)
    v = ng + b
    floor = torch.tensor(1e-6, dtype=torch.float32).to(T).double()
    vt = v if mutant == "amax_unrounded" else v.to(torch.float32).to(T).double()
    amax = torch.maximum(vt.abs().amax(-1), floor)
    return v * (127.0 / amax)[:, None], amax, ng.abs() + b.abs()


def quantize_weight(weight: torch.Tensor):
    """awq/quantize/w8a8_linear.py:154-171: s = clamp(max |w|, 1e-5) / 127 per row in the weight's dtype, q = int8(round(w / s)),
    dequant_scale = s.half().  Restated per element with float64 to check the dtype arithmetic: each step is one correctly rounded
    operation of the weight's dtype."""
    T = weight.dtype
    w = weight.cpu()
    amax = w.abs().amax(-1, keepdim=True)
    lo = torch.tensor(1e-5, dtype=torch.float32).to(T)
    s = (torch.maximum(amax, lo).double() / 127.0).to(torch.float32).to(T)
    ratio = (w.double() / s.double()).to(torch.float32).to(T)
    return torch.round(ratio.double()).to(torch.int8), s.reshape(-1).to(torch.float16)
