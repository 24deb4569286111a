"""float64 statement of soft-capped attention on a windowed packed step (awq_attn_varq_softcap and its siblings; csrc/awq_softcap.hpp):
`tests.attn_window_oracle.attention` plus `cap` and a free `scale`.

    z_j = cap * tanh(scale * (q . k_j) / cap),   then the causal / window mask by selection (a masked logit is -inf, not -cap), then softmax

The `stats` are the window oracle's (A and qk over the ATTENDED keys).  `bound` is `attn_prefill_oracle.bound` with the logit perturbation
delta enlarged by C * 2^-24 * cap: |d tanh| <= 1, so the perturbation of the raw logit -- the fp32 dot product, the scaling, the exp --
carries through the cap unchanged, and what the cap adds is the absolute error of the device tanh times cap.

The device tanh (softcap_tanh, csrc/awq_softcap.hpp) and where C comes from.  For an fp32 y the kernels evaluate

    t = fl(y * K)        K = fl(2 log2 e)                       one multiply
    e = exp2(t)          v_exp_f32, 1 ulp                       (t > 128: +inf; t < -126: 0 or a denormal)
    d = fl(1 + e)                                               one add
    r = rcp(d)           v_rcp_f32, 1 ulp
    out = fl(1 - 2 r)                                           one fma, |out| <= 1

and tanh(y) = 1 - 2 / (1 + 2^(2 log2 e * y)) exactly.  With u = 2^-24 (half an ulp of a value in [1, 2), the relative rounding error):

  1. the argument: K carries a relative error <= 0.7 u (2^-23 / 2.885) and the product one more u, so t stands for y (1 + eps) with
     |eps| <= 1.7 u, and tanh(y (1 + eps)) - tanh(y) = y eps sech^2(xi) with xi beside y.  max_x x sech^2(x) = 0.4478 (at x = 0.7717), so this
     is at most 0.77 u for every finite y -- the one place where a RELATIVE error of an unbounded argument turns into a bounded absolute one.
  2. exp2: e (1 + eta), |eta| <= 2 u.  d/de [1 - 2 / (1 + e)] = 2 / (1 + e)^2, times e eta: 2 e / (1 + e)^2 <= 1/2, so at most 1 u.
  3. the add: d in [1, 2) is rounded by at most u, d in [2^k, 2^(k+1)) by 2^k u; the result moves by 2 / d^2 times that: at most 2 u (d -> 1).
  4. rcp: r (1 + rho), |rho| <= 2 u, r <= 1; the result moves by 2 r |rho| <= 4 u.
  5. the fma rounds a value of magnitude <= 1 once: at most u / 2.

  0.77 + 1 + 2 + 4 + 0.5 = 8.27 u, with second-order terms of order u^2.  The ends: e = +inf gives d = +inf, r = 0, out = 1; e = 0 (or a
  flushed denormal, error below 2^-126) gives d = 1, r = 1, out = -1; a NaN stays a NaN through every step.

The callers add one thing in front: y = fl(s * fl(scale / cap)) for the attention, y = fl(z / cap) for logits -- at most two more relative
errors u of the argument, which by the bound of step 1 cost at most 0.9 u.  8.27 + 0.9 = 9.17, so

    |cap * device_tanh(y_device) - cap * tanh(y)| <= C * 2^-24 * cap   with   C = 10.

(The product with cap * log2 e that follows is a relative error of a logit no larger than scale * |q . k| in magnitude: `bound`'s own "+ 4".)

`mutant` switches one fault in, for the tests that prove the inputs can see it:

    nocap            z = scale * qk
    scale-outside    z = cap * tanh(qk / cap) * scale
    log2e-inside     base 2 taken inside the tanh: z = cap * tanh(scale * qk * log2 e / cap) / log2 e
    half-arg         z = cap * tanh(y / 2), y = scale * qk / cap
    cap-after-mask   the mask in front of the cap: a masked key's logit is cap * tanh(-inf) = -cap"""
from __future__ import annotations

import math

import torch

from tests import attn_prefill_oracle as P

MUTANTS = ("nocap", "scale-outside", "log2e-inside", "half-arg", "cap-after-mask")
C = 10.0          # |device tanh - tanh| <= C * 2^-24, argument roundings of the callers included (derived above); the issue's condition: C <= 16
LOG2E = 1.4426950408889634


def logits(qk, scale, cap, mutant=None):
    """float64 z for raw dot products qk; cap = inf is no cap."""
    if mutant == "nocap" or math.isinf(cap):
        return qk * scale
    if mutant == "scale-outside":
        return cap * torch.tanh(qk / cap) * scale
    if mutant == "log2e-inside":
        return cap * torch.tanh(qk * scale * LOG2E / cap) / LOG2E
    if mutant == "half-arg":
        return cap * torch.tanh(qk * scale / cap / 2)
    return cap * torch.tanh(qk * scale / cap)


def attention(q, k, v, window_left, cap, scale=None, mutant=None, stats: bool = False):
    """q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] -> out float64 [B, Sq, H, Dh]; with stats also A [B, Sq, H, Dh] and qk [B, Sq, H]."""
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = H // Hkv
    sc = float(Dh) ** -0.5 if scale is None else float(scale)
    cap = float(cap)
    dev = q.device
    i = torch.arange(Sq, device=dev)[:, None]
    j = torch.arange(Sk, device=dev)[None, :]
    p = i + (Sk - Sq)
    start = (p - int(window_left)).clamp_min(0)
    dead = (j > p) | (j < start)
    out = torch.zeros(B, Sq, H, Dh, dtype=torch.float64, device=dev)
    A = torch.zeros_like(out) if stats else None
    qk = torch.zeros(B, Sq, H, dtype=torch.float64, device=dev) if stats else None
    for b in range(B):
        for h in range(H):
            kvh = h // G
            K, V, Q = k[b, :, kvh].double(), v[b, :, kvh].double(), q[b, :, h].double()
            s = logits(Q @ K.T, sc, cap, mutant)
            if mutant == "cap-after-mask":
                s = s.masked_fill(dead, -cap)
            else:
                s = s.masked_fill(dead, float("-inf"))   # by selection: whatever a dead key's score is, NaN included
            pr = torch.softmax(s, -1)
            pr = pr.masked_fill(p < 0, 0.0)
            Vd = torch.where(torch.isfinite(V), V, torch.zeros_like(V))
            out[b, :, h] = pr @ Vd
            if stats:
                A[b, :, h] = pr @ Vd.abs()
                Kd = torch.where(torch.isfinite(K), K, torch.zeros_like(K))
                qk[b, :, h] = (Q.abs() @ Kd.abs().T).masked_fill(dead, 0.0).max(-1).values
    return (out, A, qk) if stats else out


def bound(ref, A, qk, dtype, Sk: int, Dh: int, scale: float, cap: float) -> torch.Tensor:
    """`attn_prefill_oracle.bound` with delta enlarged by C * 2^-24 * cap (cap = inf: the bound itself)."""
    u = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}[dtype]
    delta = (Dh + 4) * 2.0 ** -24 * abs(scale) * qk
    if not math.isinf(cap):
        delta = delta + C * 2.0 ** -24 * cap
    return 0.5 * P.ulp(ref, dtype) + (2 * u + 2 * Sk * 2.0 ** -24 + 2 * delta[..., None]) * A
