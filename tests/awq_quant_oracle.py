"""Oracle of the AWQ quantisation entries (awq_quantize_group, awq_clip_search): torch on the CPU, built on oracle.awq_oracle.

TEST INFRASTRUCTURE ONLY.  Piece 1 is the torch composition the kernel must reproduce bit for bit: the optional column scaling and clamp in T,
`pseudo_quantize` (quantizer.py:61-103 restated in oracle/awq_oracle.py), `from_linear`'s buffers (`wq_buffers_from_fake`) and the cdna4 pack.
Piece 2 gives the clip candidates in T and the error table of the search in float64 (the exact value) and in float32 (the yardstick the
tolerance of the kernel is sized with, tests/awq_quant_cases.py).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import awq_oracle as O

GROUP = 128


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit patterns of a tensor as integers of its width (so that -0.0 != 0.0 and NaN == NaN in comparisons)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def scale_buffers(s: torch.Tensor, z: torch.Tensor, K: int):
    """from_linear's (qmodule.py:155-197) `scales` and `scaled_zeros` [gpad, N] from the grid's per-group scales / zeros [N, K/128]: zero pad
    rows, scaled_zeros = -(T(scale) * float(int(zero))) rounded to T.  (For n_bit 4 this equals what wq_buffers_from_fake returns.)"""
    T, N, G = s.dtype, s.shape[0], s.shape[1]
    gp = O.padded_groups(K, GROUP)
    qs = torch.zeros((N, gp), dtype=T)
    qs[:, :G] = s
    sz = torch.zeros_like(qs)
    sz[:, :G] = -(s * z.to(torch.int32).to(torch.float32)).to(T)
    return qs.t().contiguous(), sz.t().contiguous()


def quantize_group(w: torch.Tensor, col_scale=None, clip_max=None, n_bit: int = 4) -> dict:
    """Everything awq_quantize_group can write, for w T [N, K] on the CPU (col_scale T [K], clip_max T [N, K/128]):
    w_fake T [N, K], zeros T [N, K/128], scales / scaled_zeros T [gpad, N], and for n_bit 4 the integers from_linear recovers with
    qweight_v2 / qweight_cdna4 int16 [N/4, K] (None where N is not a multiple of 8 / 16)."""
    N, K = w.shape
    G = K // GROUP
    v = w
    if col_scale is not None:
        v = v * col_scale.view(1, K)                          # one rounding to T
    if clip_max is not None:
        c = clip_max.view(N, G, 1)
        v = torch.clamp(v.reshape(N, G, GROUP), -c, c).reshape(N, K)
    fake, s, z = O.pseudo_quantize(v.contiguous(), n_bit, GROUP)
    out = dict(w_fake=fake / col_scale.view(1, K) if col_scale is not None else fake, zeros=z, s=s)
    out["scales"], out["scaled_zeros"] = scale_buffers(s, z, K)
    out["intweight"] = iw = O.intweight_from_fake(fake, s, z, GROUP)
    out["qweight_v2"] = out["qweight_cdna4"] = None
    if n_bit == 4 and N % 8 == 0:
        qw, qs, sz, iw2 = O.wq_buffers_from_fake(fake, s, z, GROUP, 4)
        assert torch.equal(iw2, iw) and torch.equal(bits(qs), bits(out["scales"])) and torch.equal(bits(sz), bits(out["scaled_zeros"]))
        out["qweight_v2"] = qw
        if N % 16 == 0:
            out["qweight_cdna4"] = torch.from_numpy(O.pack_cdna4(iw.numpy()))
    return out


def shrink_factor(i: int, n_grid: int) -> float:
    """auto_clip.py:42 writes `org_max_val * (1 - i_s / n_grid)`: a Python double.  The kernel receives it rounded to fp32."""
    return float(np.float32(1 - i / n_grid))


def clip_candidates(w: torch.Tensor, n_bit: int = 4, n_grid: int = 20, n_steps: int = 10):
    """-> (mv T [n_steps, N, G], q T [n_steps, N, K]).  mv_i = round_T(fp32(m) * fp32(1 - i / n_grid)) with m = amax|w| of the group: the product is
    taken in fp32 with the factor as an fp32 scalar (the bits a GPU tensor-times-Python-scalar gives), then rounded to T once.  For n_grid 20 the
    fp32 factors are 1, 0.95, 0.9, ... with bit patterns 0x3f800000, 0x3f733333, 0x3f666666, 0x3f59999a, 0x3f4ccccd, 0x3f400000, 0x3f333333,
    0x3f266666, 0x3f19999a, 0x3f0ccccd.  q_i is the grid applied to clamp(w, -mv_i, mv_i) in T."""
    N, K = w.shape
    G = K // GROUP
    g = w.reshape(N, G, GROUP)
    m = g.abs().amax(dim=-1)
    mvs, qs = [], []
    for i in range(n_steps):
        mv = (m.float() * torch.tensor(shrink_factor(i, n_grid), dtype=torch.float32)).to(w.dtype)
        cur = torch.clamp(g, -mv.unsqueeze(-1), mv.unsqueeze(-1)).reshape(N, K).contiguous()
        mvs.append(mv)
        qs.append(O.pseudo_quantize(cur, n_bit, GROUP)[0])
    return torch.stack(mvs), torch.stack(qs)


def clip_error_table(w: torch.Tensor, x: torch.Tensor, q: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """err[n, g, i] = (1/S) sum_t (x_t . q_i[n, g] - x_t . w[n, g])^2 evaluated in `dtype` (float64: the exact value; float32: the same formula
    as torch evaluates it on the CPU) from the T inputs.  w [N, K], x [S, K], q [n_steps, N, K]."""
    N, K = w.shape
    S, G = x.shape[0], K // GROUP
    xg = x.to(dtype).reshape(S, G, GROUP)
    ow = torch.einsum("sgk,ngk->nsg", xg, w.to(dtype).reshape(N, G, GROUP))
    errs = []
    for i in range(q.shape[0]):
        oq = torch.einsum("sgk,ngk->nsg", xg, q[i].to(dtype).reshape(N, G, GROUP))
        errs.append(((oq - ow) ** 2).sum(dim=1) / S)
    return torch.stack(errs, dim=-1)  # [N, G, n_steps]


def first_strict_min(err: torch.Tensor) -> torch.Tensor:
    """auto_clip.py:52-54: the first i whose error is strictly below 1e9 and every earlier one; 0 if there is none."""
    best = torch.full(err.shape[:-1], 1e9, dtype=err.dtype)
    idx = torch.zeros(err.shape[:-1], dtype=torch.int32)
    for i in range(err.shape[-1]):
        take = err[..., i] < best
        best = torch.where(take, err[..., i], best)
        idx = torch.where(take, torch.full_like(idx, i), idx)
    return idx


def amax_of_clamped_is_clamped_amax(w: torch.Tensor, mv: torch.Tensor) -> bool:
    """The extremes of a clamped group are the clamped extremes of the group (clamp is monotone), which lets the kernel reduce once per cell."""
    N, K = w.shape
    g = w.reshape(N, K // GROUP, GROUP)
    c = mv.unsqueeze(-1)
    cl = torch.clamp(g, -c, c)
    return bool(torch.equal(cl.amax(-1), torch.clamp(g.amax(-1), -mv, mv)) and torch.equal(cl.amin(-1), torch.clamp(g.amin(-1), -mv, mv)))
