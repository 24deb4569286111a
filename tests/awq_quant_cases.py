"""Inputs and constants shared by the AWQ quantisation tests (tests/test_awq_quant_host.py, tests/test_gpu_awq_quant.py)."""
from __future__ import annotations

import functools

import torch

GROUP = 128
N_GRID, N_STEPS = 20, 10

# piece 1: (N, K).  K 256 / 384 have pad rows in scales / scaled_zeros (gpad 8 > 2, 3 groups); N 272 is no multiple of 32, 64, 128 or 256
QUANT_SHAPES = ((16, 128), (16, 256), (48, 384), (272, 256))
# piece 2: (N, K, S).  S 1 / 3: a fraction of a token tile; 64: whole tiles; 513: seventeen tiles, the last with one token; 272 rows: 8.5 row tiles
CLIP_SHAPES = ((16, 128, 1), (32, 256, 3), (48, 384, 64), (32, 256, 513), (272, 256, 40))

# The tolerance of the clip search's error table, in units of max_i err64[n, g, :] (check 3 of the issue).  D is the largest deviation of the
# float32 torch-CPU evaluation of the same formula from the float64 one over CLIP_SHAPES x {fp16, bf16} x the inputs below
# (tests/test_awq_quant_host.py re-measures it; another CPU's fp32 sum order moves it a little); the kernel sums in another order and the cancellation in
# x.q - x.w amplifies an order change by about the factor measured in D, so it gets FACTOR times D.
D_F32 = {torch.float16: 5.7e-6, torch.bfloat16: 2.9e-6}   # measured 5.60e-6 and 2.88e-6, both on case (32, 256, 3)
FACTOR = 8.0
N_BIT3_CASE = (48, 384, 64)  # the clip-search case that is also run with n_bit 3
TOL = {T: FACTOR * d for T, d in D_F32.items()}
DECISIVE_FRACTION = 0.95
X_SEED = 2  # (with one token and 16 cells a single near-tie of the fp64 oracle breaks the 95 % condition: seeds 0 and 1 have one)

PLANTED = ("zero", "constant", "positive", "negative", "outlier", "ties", "subnormal")
# In an all-zero group every clip candidate has error 0 and in a constant one every candidate quantises alike, so no index is decisive there; with
# 16 cells in the smallest case one such cell breaks the 95 % condition.  The clip-search cases leave these two kinds out; what the search must
# answer on them (step 0) is pinned by test_gpu_awq_quant.py's planted-cell test.
DEGENERATE_FOR_CLIP = ("zero", "constant")


def planted_cell(kind_index: int, G: int):
    """(row, group) of planted group number kind_index."""
    return kind_index, kind_index % G


@functools.lru_cache(maxsize=None)
def make_weight(N: int, K: int, dtype, seed: int = 0, clip_spikes: bool = False) -> torch.Tensor:
    """N(0, 0.02) in T with the planted groups of PLANTED in rows 0..6 (group = row % G).  clip_spikes: every 5th row's every 37th column x 6
    (the clip search's inputs).  The returned tensor is shared: do not write to it."""
    gen = torch.Generator().manual_seed(1000 * seed + N + K)
    w = (torch.randn(N, K, generator=gen) * 0.02)
    if clip_spikes:
        w[::5, ::37] *= 6
    G = K // GROUP
    for i, kind in enumerate(PLANTED):
        r, g = planted_cell(i, G)
        if r >= N or (clip_spikes and kind in DEGENERATE_FOR_CLIP):
            continue
        sl = slice(g * GROUP, (g + 1) * GROUP)
        if kind == "zero":
            w[r, sl] = 0
        elif kind == "constant":
            w[r, sl] = 0.0123
        elif kind == "positive":
            w[r, sl] = w[r, sl].abs()
        elif kind == "negative":
            w[r, sl] = -w[r, sl].abs()
        elif kind == "outlier":
            w[r, g * GROUP + 41] = 0.6          # 30 sigma
        elif kind == "ties":
            # extremes -7 s and 8 s with s = 2^-8: scale = s exactly, zero = 7; every other value is (j + 0.5) s, a round-half-even tie
            s = 2.0 ** -8
            j = torch.arange(GROUP) % 15 - 7
            w[r, sl] = (j + 0.5) * s
            w[r, g * GROUP] = -7 * s
            w[r, g * GROUP + 1] = 8 * s
        elif kind == "subnormal":
            w[r, sl] = torch.randn(GROUP, generator=gen) * 2e-5   # below fp16's smallest normal (6.1e-5): subnormal values, range above 1e-5
    return w.to(dtype)


@functools.lru_cache(maxsize=None)
def make_x(S: int, K: int, dtype, seed: int = 0) -> torch.Tensor:
    """N(0, 1) with every 29th channel x 8."""
    gen = torch.Generator().manual_seed(77 + 1000 * seed + S + K)
    x = torch.randn(S, K, generator=gen)
    x[:, ::29] *= 8
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def make_col_scale(K: int, dtype, seed: int = 0) -> torch.Tensor:
    """values in [0.25, 4], none a power of two"""
    gen = torch.Generator().manual_seed(5 + seed + K)
    s = (0.25 + 3.75 * torch.rand(K, generator=gen)).to(dtype)
    pow2 = torch.frexp(s.float())[0] == 0.5
    return torch.where(pow2, torch.tensor(1.37, dtype=dtype), s)


@functools.lru_cache(maxsize=None)
def make_clip_max(N: int, K: int, dtype, seed: int = 0) -> torch.Tensor:
    """[N, K/128]: the group's amax times a factor in [0.5, 1.1] (some groups are not clipped at all), 0 for the all-zero group."""
    w = make_weight(N, K, dtype, seed)
    gen = torch.Generator().manual_seed(9 + seed + N * K)
    m = w.reshape(N, K // GROUP, GROUP).abs().amax(-1).float()
    return (m * (0.5 + 0.6 * torch.rand(N, K // GROUP, generator=gen))).to(dtype)


@functools.lru_cache(maxsize=None)
def clip_reference(N: int, K: int, S: int, dtype, n_bit: int = 4):
    """The oracle's answers for one clip-search case, computed once: dict(w, x, mv [steps, N, G], q, err64, err32, idx64)."""
    from tests import awq_quant_oracle as QO

    w, x = make_weight(N, K, dtype, 0, True), make_x(S, K, dtype, X_SEED)
    mv, q = QO.clip_candidates(w, n_bit, N_GRID, N_STEPS)
    err64 = QO.clip_error_table(w, x, q, torch.float64)
    err32 = QO.clip_error_table(w, x, q, torch.float32)
    return dict(w=w, x=x, mv=mv, q=q, err64=err64, err32=err32, idx64=QO.first_strict_min(err64))


def table_deviation(err, err64) -> float:
    """check 3's metric: max over cells and steps of |err - err64| / max_i err64[n, g, :] (cells whose errors are all zero must be met exactly)."""
    scale = err64.max(dim=-1, keepdim=True).values
    dev = (err.double() - err64).abs()
    assert bool((dev[(scale == 0).expand_as(dev)] == 0).all())
    return float((dev / scale.clamp(min=1e-300)).max())


def decisive_cells(err64, tol: float):
    """-> (decisive [N, G] bool, allowed [N, G, steps] bool): a cell is decisive if the fp64 runner-up exceeds the fp64 best by more than
    2 tol max_i err64; on the others every index within that distance of the best is allowed."""
    scale = err64.max(dim=-1, keepdim=True).values
    best = err64.min(dim=-1, keepdim=True).values
    allowed = err64 <= best + 2 * tol * scale
    return allowed.sum(-1) == 1, allowed
