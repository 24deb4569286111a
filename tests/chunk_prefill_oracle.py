"""float64 restatement of rope_kv_store (csrc/awq_attn_chunk_cdna4.hip): tests/rope_oracle.py's with-pos rotation plus the index map of the
FasterTransformer caches, written as flat offsets (not as the reference's permute / slice-assign, which tests/test_chunk_prefill_host.py
compares it with):

    k_cache [Bc, Hkv, Dh/8, Lmax, 8]   element (b, kvh, c) of position p lies at (((b Hkv + kvh) Dh/8 + c // 8) Lmax + p) 8 + c % 8
    v_cache [Bc, Hkv, Lmax, Dh]        element (b, kvh, c) of position p lies at ((b Hkv + kvh) Lmax + p) Dh + c
"""
from __future__ import annotations

import torch

from tests import rope_oracle as R


def split_qkv(qkv: torch.Tensor, H: int, Hkv: int):
    """qkv [B, S, (H + 2 Hkv) Dh] -> the views q [B, S, H, Dh], k, v [B, S, Hkv, Dh] (tinychat's fused_attn.py:236-246)."""
    B, S, W = qkv.shape
    Dh = W // (H + 2 * Hkv)
    x = qkv.view(B, S, H + 2 * Hkv, Dh) if qkv.is_contiguous() else qkv.reshape(B, S, H + 2 * Hkv, Dh)
    return x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]


def ft_offsets(B: int, S: int, Hkv: int, Dh: int, Lmax: int, start_pos: int, device=None):
    """Flat offsets into k_cache and v_cache of element (b, s, kvh, c) of a [B, S, Hkv, Dh] tensor stored at positions start_pos + s."""
    b = torch.arange(B, device=device)[:, None, None, None]
    p = start_pos + torch.arange(S, device=device)[None, :, None, None]
    kvh = torch.arange(Hkv, device=device)[None, None, :, None]
    c = torch.arange(Dh, device=device)[None, None, None, :]
    k_off = (((b * Hkv + kvh) * (Dh // 8) + c // 8) * Lmax + p) * 8 + c % 8
    v_off = ((b * Hkv + kvh) * Lmax + p) * Dh + c
    return k_off, v_off


def rope_kv_store(qkv: torch.Tensor, freqs: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, start_pos: int, H: int, Hkv: int):
    """-> (q_ref float64 [B, S, H, Dh], q_mag, k_ref float64 cache, k_mag cache, v cache): the caches are copies of k_cache / v_cache
    (k in float64) with the chunk written at its flat offsets; k_mag is zero wherever nothing rotated was written."""
    xq, xk, xv = split_qkv(qkv, H, Hkv)
    B, S, _, Dh = xk.shape
    Lmax = v_cache.shape[2]
    q_ref, q_mag = R.fused_rope_with_pos(xq, freqs)
    k_rot, k_rot_mag = R.fused_rope_with_pos(xk, freqs)
    k_off, v_off = ft_offsets(B, S, Hkv, Dh, Lmax, start_pos, device=qkv.device)
    k_ref = k_cache.double().clone()
    k_mag = torch.zeros_like(k_ref)
    v_new = v_cache.clone()
    k_ref.view(-1)[k_off.reshape(-1)] = k_rot.reshape(-1)
    k_mag.view(-1)[k_off.reshape(-1)] = k_rot_mag.reshape(-1)
    v_new.view(-1)[v_off.reshape(-1)] = xv.reshape(-1)
    return q_ref, q_mag, k_ref, k_mag, v_new


def gather_ft(k_cache: torch.Tensor, v_cache: torch.Tensor, B: int, kv_start: int, Sk: int):
    """The contiguous [B, Sk, Hkv, Dh] copies of cache positions kv_start .. kv_start + Sk - 1 (fused_attn.py:456-472)."""
    Hkv, Dh = v_cache.shape[1], v_cache.shape[3]
    k = k_cache[:B, :, :, kv_start:kv_start + Sk, :].permute(0, 3, 1, 2, 4).reshape(B, Sk, Hkv, Dh).contiguous()
    v = v_cache[:B, :, kv_start:kv_start + Sk, :].transpose(2, 1).reshape(B, Sk, Hkv, Dh).contiguous()
    return k, v


def scatter_ft(k: torch.Tensor, v: torch.Tensor, Bc: int, Lmax: int, kv_start: int, fill=float("nan")):
    """FT caches [Bc, ...] holding `fill` everywhere except k / v [B, Sk, Hkv, Dh] at positions kv_start .. kv_start + Sk - 1."""
    B, Sk, Hkv, Dh = k.shape
    kc = torch.full((Bc, Hkv, Dh // 8, Lmax, 8), fill, dtype=k.dtype, device=k.device)
    vc = torch.full((Bc, Hkv, Lmax, Dh), fill, dtype=v.dtype, device=v.device)
    vc[:B, :, kv_start:kv_start + Sk, :] = v.transpose(1, 2)
    kc[:B, :, :, kv_start:kv_start + Sk, :] = k.reshape(B, Sk, Hkv, Dh // 8, 8).permute(0, 2, 3, 1, 4)
    return kc, vc
