"""float64 statement of prefill attention as tinychat asks for it through flash_attn_func (llama.py:218, fused_attn.py:477,539):

    q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] -> out [B, Sq, H, Dh]
    O = softmax(scale * Q K^T + mask) V, plain softmax; query head h reads KV head h // (H // Hkv)
    causal: row i attends keys j <= i + (Sk - Sq) (bottom-right aligned, flash-attn >= 2.1)

tests.attn_oracle.causal_attention is the square single-head special case.  Runs on the device of its inputs (the CPU tests call it on
CPU tensors, the GPU tests on GPU tensors so that S = 8192 stays affordable), one (batch, head) and at most `rows` query rows at a time:
nothing of size B x H x Sq x Sk is held.

`mutant` switches one fault in, for the tests that prove the needle inputs can see it:
    mask+1 / mask-1   the causal limit moved by one in either direction
    topleft           the mask aligned top-left (j <= i) instead of bottom-right
    kvh+1             the next KV head
    droptile          the last 64-key tile of K / V not visited
    unscaled          the softmax scale ignored (taken as the default Dh ** -0.5)
"""
from __future__ import annotations

import torch

MUTANTS = ("mask+1", "mask-1", "topleft", "kvh+1", "droptile", "unscaled")
TILE = 64


def attention(q, k, v, scale=None, causal=False, mutant=None, rows: int = 1024, stats: bool = False):
    """out float64 [B, Sq, H, Dh]; with stats also A = sum_j p_j |v_j| / sum_j p_j [B, Sq, H, Dh] and
    qk = max_j sum_d |q_d k_jd| [B, Sq, H] (over the attended keys)."""
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = H // Hkv
    sc = float(Dh) ** -0.5 if (scale is None or mutant == "unscaled") else float(scale)
    shift = 0 if mutant == "topleft" else Sk - Sq
    shift += {"mask+1": 1, "mask-1": -1}.get(mutant, 0)
    n_k = (Sk - 1) // TILE * TILE if mutant == "droptile" else Sk
    dev = q.device
    out = torch.zeros(B, Sq, H, Dh, dtype=torch.float64, device=dev)
    A = torch.zeros_like(out) if stats else None
    qk = torch.zeros(B, Sq, H, dtype=torch.float64, device=dev) if stats else None
    j = torch.arange(n_k, device=dev)[None, :]
    for b in range(B):
        for h in range(H):
            kvh = h // G
            if mutant == "kvh+1":
                kvh = (kvh + 1) % Hkv
            K = k[b, :n_k, kvh].double()
            V = v[b, :n_k, kvh].double()
            for r0 in range(0, Sq, rows):
                Q = q[b, r0:r0 + rows, h].double()
                s = (Q @ K.T) * sc
                if causal:
                    i = torch.arange(r0, r0 + Q.shape[0], device=dev)[:, None]
                    dead = j > i + shift
                    s = s.masked_fill(dead, float("-inf"))
                p = torch.softmax(s, -1)  # (a row with nothing attended -- only under a mutant -- comes out NaN: it fails the comparison)
                out[b, r0:r0 + rows, h] = p @ V
                if stats:
                    A[b, r0:r0 + rows, h] = p @ V.abs()
                    m = Q.abs() @ K.abs().T
                    if causal:
                        m = m.masked_fill(dead, 0.0)
                    qk[b, r0:r0 + rows, h] = m.max(-1).values
    return (out, A, qk) if stats else out


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at |x| (float64 in, float64 out), subnormal spacing at the bottom."""
    fi = torch.finfo(dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    a = x.abs().clamp_min(fi.tiny)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - mant)


def bound(ref, A, qk, dtype, Sk: int, Dh: int, scale: float) -> torch.Tensor:
    """Elementwise |out - ref| allowed for a flash loop with fp32 scores and accumulation and weights rounded to T once:
        1/2 ulp_T(ref) + (2 u_T + 2 Sk 2^-24 + 2 delta) A,   delta = (Dh + 4) 2^-24 scale max_j sum_d |q_d k_jd|
    u_T: the rounding of a weight (numerator and denominator each carry it), Sk 2^-24: worst-case fp32 accumulation of either sum,
    delta: the perturbation of a logit from the fp32 dot product, the scaling and exp."""
    u = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}[dtype]
    delta = (Dh + 4) * 2.0 ** -24 * abs(scale) * qk
    return 0.5 * ulp(ref, dtype) + (2 * u + 2 * Sk * 2.0 ** -24 + 2 * delta[..., None]) * A
