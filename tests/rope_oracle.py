"""float64 restatements of the two rotary-embedding exports tinychat calls on a prompt.

fused_rope_with_pos (awq/kernels/csrc/rope_new/fused_rope_with_pos.cu:33-72, 263-333): input [n0, n1, h, d]; the block of (i0, i1) runs
with blockIdx.x = i0, blockIdx.y = i1, gridDim.x = n0 and reads its angles at freqs[(b_id * s + s_id) * d2 + c] = flat[(i1 * n0 + i0) * d2 + c]
(:45); x_rot = -x[c + d2/2] for c < d2/2, x[c - d2/2] above (:51-55); out = x cos + x_rot sin (:55); columns >= d2 are copied (:60-70).

rotary_embedding_neox (awq/kernels/csrc/position_embedding/pos_encoding_kernels.cu:12-87): query / key [tokens, heads, head_size], the
cache row of positions[token] holds cos (first rot_dim / 2) | sin; x' = x cos - y sin, y' = y cos + x sin with y = x[.. + rot_dim / 2].
"""
from __future__ import annotations

import torch


def fused_rope_with_pos(x: torch.Tensor, freqs: torch.Tensor):
    """-> (ref float64 [n0, n1, h, d], mag = |x| + |x_rot| float64, zero on the copied columns)."""
    n0, n1, h, d = x.shape
    d2 = freqs.shape[-1]
    flat = freqs.double().reshape(-1)
    i0 = torch.arange(n0, device=x.device)[:, None]
    i1 = torch.arange(n1, device=x.device)[None, :]
    base = ((i1 * n0 + i0) * d2)[..., None] + torch.arange(d2, device=x.device)  # [n0, n1, d2]
    ang = flat[base][:, :, None, :]
    xd = x.double()
    rot = torch.cat([-xd[..., d2 // 2:d2], xd[..., :d2 // 2]], -1)
    ref = xd.clone()
    ref[..., :d2] = xd[..., :d2] * torch.cos(ang) + rot * torch.sin(ang)
    mag = torch.zeros_like(xd)
    mag[..., :d2] = xd[..., :d2].abs() + rot.abs()
    return ref, mag


def rotary_embedding_neox(positions: torch.Tensor, x: torch.Tensor, head_size: int, cache: torch.Tensor):
    """x [..., heads, head_size] -> (ref float64 of the same shape, mag)."""
    rot = cache.shape[1]
    e = rot // 2
    heads = x.shape[-2]
    xd = x.double().reshape(-1, heads, head_size)
    cs = cache.double()[positions.reshape(-1)]
    c, s = cs[:, None, :e], cs[:, None, e:]
    a, b = xd[..., :e], xd[..., e:rot]
    ref = xd.clone()
    ref[..., :e] = a * c - b * s
    ref[..., e:rot] = b * c + a * s
    mag = torch.zeros_like(xd)
    mag[..., :e] = a.abs() + b.abs()
    mag[..., e:rot] = a.abs() + b.abs()
    return ref.reshape(x.shape), mag.reshape(x.shape)
