"""float64 restatement of FasterTransformer's masked multi-head attention decode step, as tinychat calls it through
awq_inference_engine.single_query_attention (awq/kernels/csrc/attention/ft_attention.cpp:112-185 and
decoder_masked_multihead_attention_template.hpp, "MMHA" below).

    tlength      = length_per_sample[b] if given, else timestep                        MMHA :975-978
    first_step   = max(0, tlength + 1 - Lmax), cache index pos % Lmax                   MMHA :979-980
    query head h reads KV head h // (H // Hkv)                                          MMHA :944-945
    rotary       GPT-J pairs (2i, 2i + 1) (MMHA :1080-1086), NeoX pairs (i, i + rot / 2) (MMHA :1088-1130),
                 angle = (t * scale) / base ** (2i / rot) in fp32 (..._utils.h:1282-1287), the rotated q / k rounded to T
    scores       q . k / sqrt(Dh) + slope[h] * (pos - tlength)                          MMHA :1335-1345
    softmax      exp(s - max) / (sum + 1e-6)                                            MMHA :1399
    cache write  rotated k (as T) and v at tlength % Lmax                               MMHA :1029, :1540

Everything after the rotation is float64: the kernel's fp32 softmax / P.V (a deliberate deviation from FT, which rounds the
logits to T) is compared against it.
"""
from __future__ import annotations

import numpy as np
import torch


def rotary_pairs(rot: int, neox: bool):
    half = rot // 2
    i = np.arange(half)
    return (i, i + half) if neox else (2 * i, 2 * i + 1)


def rotate(x: torch.Tensor, t: int, rot: int, base: float, scale: float, neox: bool, emulate_fp32: bool = True) -> torch.Tensor:
    """Rotary embedding of x [..., Dh] at position t over the first `rot` dims.  emulate_fp32: the angle, cos / sin and the
    rotation in fp32 and the result rounded to x.dtype (the kernel's arithmetic); else all in float64, unrounded."""
    if rot == 0:
        return x.clone()
    i0, i1 = rotary_pairs(rot, neox)
    zid = 2 * np.arange(rot // 2)
    ft = np.float32 if emulate_fp32 else np.float64
    ang = (ft(t) * ft(scale)) / np.power(ft(base), zid.astype(ft) / ft(rot))
    c, s = np.cos(ang).astype(ft), np.sin(ang).astype(ft)
    xf = x.double().numpy().astype(ft)
    y = xf.copy()
    x0, x1 = xf[..., i0], xf[..., i1]
    y[..., i0] = c * x0 - s * x1
    y[..., i1] = c * x1 + s * x0
    out = torch.from_numpy(y.astype(np.float64))
    return out.to(x.dtype) if emulate_fp32 else out


def angle_slack(x: torch.Tensor, t: int, rot: int, base: float, scale: float, neox: bool) -> torch.Tensor:
    """Per-element change of the rotated x [Dh] when the fp32 angle moves by two of its ulps: the kernel's powf / cosf / sinf and
    numpy's need not round alike, and at large t one angle ulp is already a visible fraction of an fp16 / bf16 ulp."""
    out = torch.zeros(x.shape[-1], dtype=torch.float64)
    if rot == 0:
        return out
    i0, i1 = rotary_pairs(rot, neox)
    zid = 2 * np.arange(rot // 2)
    ang = (np.float32(t) * np.float32(scale)) / np.power(np.float32(base), zid.astype(np.float32) / np.float32(rot))
    d = 2.0 * np.spacing(np.abs(ang).astype(np.float32)).astype(np.float64)
    mag = x.double().numpy()
    pair = np.abs(mag[i0]) + np.abs(mag[i1])
    out[i0] = torch.from_numpy(d * pair)
    out[i1] = torch.from_numpy(d * pair)
    return out


def k_cache_rows(k_cache: torch.Tensor, b: int, kvh: int, idx) -> torch.Tensor:
    """K vectors [n, Dh] at cache indices idx from the FT layout [Bc, Hkv, Dh/8, Lmax, 8]."""
    kc = k_cache[b, kvh][:, idx, :]  # [Dh/8, n, 8]
    return kc.permute(1, 0, 2).reshape(len(idx), -1)


def decode(q, k, v, k_cache, v_cache, length_per_sample=None, alibi_slopes=None, timestep: int = 0, rot: int = 0,
           base: float = 10000.0, scale: float = 1.0, neox: bool = True):
    """One decode step on CPU tensors: returns (out float64 [B, H, Dh], k_rot [B, Hkv, Dh] in T, q_rot [B, H, Dh] in T).
    The caches are read only (the written entries are taken from k_rot / v)."""
    B, H, Dh = q.shape
    Hkv, Lmax = v_cache.shape[1], v_cache.shape[2]
    G = H // Hkv
    out = torch.zeros(B, H, Dh, dtype=torch.float64)
    k_rot = torch.empty(B, Hkv, Dh, dtype=q.dtype)
    q_rot = torch.empty(B, H, Dh, dtype=q.dtype)
    for b in range(B):
        t = int(length_per_sample[b]) if length_per_sample is not None else int(timestep)
        first = max(0, t + 1 - Lmax)
        pos = np.arange(first, t + 1)
        idx = pos % Lmax
        qr = rotate(q[b], t, rot, base, scale, neox)
        kr = rotate(k[b], t, rot, base, scale, neox)
        q_rot[b], k_rot[b] = qr, kr
        for kvh in range(Hkv):
            K = k_cache_rows(k_cache, b, kvh, idx).double()
            V = v_cache[b, kvh][idx].double()
            K[-1], V[-1] = kr[kvh].double(), v[b, kvh].double()
            for g in range(G):
                h = kvh * G + g
                s = (K @ qr[h].double()) / np.sqrt(Dh)
                if alibi_slopes is not None:
                    s = s + float(alibi_slopes[h]) * torch.from_numpy((pos - t).astype(np.float64))
                p = torch.exp(s - s.max())
                out[b, h] = (p @ V) / (p.sum() + 1e-6)
    return out, k_rot, q_rot


def to_ft_k_cache(K: torch.Tensor) -> torch.Tensor:
    """[Bc, Hkv, L, Dh] -> the FT layout [Bc, Hkv, Dh/8, L, 8]."""
    Bc, Hkv, L, Dh = K.shape
    return K.reshape(Bc, Hkv, L, Dh // 8, 8).permute(0, 1, 3, 2, 4).contiguous()


def causal_attention(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """Full causal softmax attention in float64: Q [T, Dh], K / V [T, Dh] -> [T, Dh]."""
    T, Dh = Q.shape
    s = (Q.double() @ K.double().T) / np.sqrt(Dh)
    s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    return torch.softmax(s, -1) @ V.double()


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at |x| (float64 in, float64 out), subnormal spacing at the bottom."""
    fi = torch.finfo(dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    a = x.abs().clamp_min(fi.tiny)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - mant)
