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
"""
from __future__ import annotations

import torch


def acc_exact(x_i8: torch.Tensor, w_i8: torch.Tensor) -> torch.Tensor:
    """x [M, K] . w [N, K]^T as int64; computed in float64, exact since |acc| <= K * 2^14 < 2^53."""
    return (x_i8.cpu().double() @ w_i8.cpu().double().t()).round().long()


def gemm_f64(acc: torch.Tensor, wscales, ascales, bias=None):
    """-> (e float64 [M, N], mag = |acc ws as| + |bias|)."""
    p = acc.double() * wscales.cpu().double()[None, :] * ascales.cpu().double()[:, None]
    b = torch.zeros_like(p) if bias is None else bias.cpu().double()[None, :].expand_as(p)
    return p + b, p.abs() + b.abs()


def gemm_f32(acc: torch.Tensor, wscales, ascales, bias=None) -> torch.Tensor:
    """The specified fp32 epilogue, step by step (float32 [M, N], not yet rounded to fp16).  The fused multiply-add is evaluated in
    float64 (the product of two float32 is exact there) and rounded to float32."""
    a32 = acc.to(torch.float32)  # int -> float32, nearest-even
    ws, as_ = wscales.cpu().float()[None, :], ascales.cpu().float()[:, None]
    if bias is None:
        return a32 * (ws * as_)
    t = a32 * ws
    return (t.double() * as_.double() + bias.cpu().double()[None, :]).to(torch.float32)


def sat_s8(y: torch.Tensor) -> torch.Tensor:
    """float_to_int8_rn: nearest-even, saturating, NaN -> 0."""
    y = torch.where(torch.isnan(y), torch.zeros_like(y), y)
    return torch.round(y).clamp_(-128, 127).to(torch.int8)


def quant_per_token(x: torch.Tensor):
    """x T [M, K] -> (q int8 [M, K], scale fp16 [M]) in IEEE float32."""
    xf = x.cpu().float()
    amax = xf.abs().amax(-1)
    scale = (amax / 127.0).to(torch.float16)
    inv = (torch.full_like(amax, 127.0) / amax)[:, None]  # inf for an all-zero row: 0 * inf = NaN -> 0
    return sat_s8(xf * inv), scale


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


def gelu_candidates(x: torch.Tensor, delta: float):
    """-> (g_lo, g_hi) fp16: gelu_fast(x) with tanh rounded to fp16 from tanh(u) (1 - delta) and tanh(u) (1 + delta).  Where the two
    agree the rounding of tanh is decided and so is g; where they differ, either neighbour is a correct result."""
    u, hx = gelu_fast_steps(x)
    th = torch.tanh(u.double())
    t_lo, t_hi = (th * (1.0 - delta)).to(torch.float32).to(_H), (th * (1.0 + delta)).to(torch.float32).to(_H)
    return gelu_from_tanh(hx, t_lo), gelu_from_tanh(hx, t_hi)


def gelu_quant_from_tmp(g: torch.Tensor):
    """g fp16 [M, K] (the kernel's tmp) -> (q int8, scale fp16 [M]); the quantisation stage of act.cu:45-68."""
    g = g.cpu()
    t = torch.where(g > torch.tensor(0.0001, dtype=torch.float32).to(_H), g, -g).float()
    amax = t.amax(-1).clamp_min(0.0) + 0.0  # amax_val starts at +0 (and -0 + 0 = +0: the sign of 127 / amax matters when amax is 0)
    scale = (amax / 127.0).to(_H)
    inv = (torch.full_like(amax, 127.0) / amax).to(_H)[:, None]
    return sat_s8(_hmul(inv.expand_as(g), g).float()), scale


def layernorm_quant_f64(x, gamma, beta, eps: float, per_token: bool, scaling=None):
    """-> (y64 [M, K]: the unrounded value whose nearest integer is q, amax64 [M] or None, mag = |n gamma| + |beta| [M, K]).
    n = (x - mean) rsqrt(var + eps) in float64; amax is taken over v rounded to x's dtype (layernorm.cu:146-150)."""
    T = x.dtype
    xd = x.cpu().double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    ng = (xd - mean) / torch.sqrt(var + eps) * gamma.cpu().double()[None, :]
    if not per_token:
        return ng * float(scaling.cpu().float()[0]), None, ng.abs()
    b = torch.zeros_like(ng) if beta is None else beta.cpu().double()[None, :].expand_as(ng)
    v = ng + b
    floor = torch.tensor(1e-6, dtype=torch.float32).to(T).double()
    amax = torch.maximum(v.to(torch.float32).to(T).double().abs().amax(-1), floor)
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
