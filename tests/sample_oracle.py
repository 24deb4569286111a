"""numpy restatement of the device-sampling contract (include/awq_cdna4.h: awq_sample_logits; DESIGN.md "Sampling"), and the builders of the test
rows.

Per row, x_v is computed in np.float32 exactly as the kernel computes it (the dtype's value, an IEEE division by the temperature, the
repetition penalty's multiply or divide): the keys the kernel compares are bit-equal to this x.  Masses m_v = exp(x_v - max x) and every sum of
them are float64 here; the kernel has fp32 `expf` and 2^-40 fixed point.  The two agree on a token whenever no threshold sits close to the
quantity it is compared with, so the oracle returns, beside the token, the row's MARGIN: the smallest distance between

  * p and any S(y) = (mass of the tokens with x_w > y) / Z          (in units of the row's mass Z), and
  * u Zk and the two prefix sums C either side of it                (in units of the kept mass Zk; the target is compared with nothing below the
                                                                    first prefix or above the last one, so those ends do not count).

Top-k compares integer counts and greedy compares keys: both are exact and have no margin.

The tests demand equality with the oracle on every row whose margin is at least MARGIN = 1e-4.  Derived, not measured: the exponent's argument
x - max has magnitude up to 64 and is rounded twice in fp32 (the subtraction, and the argument reduction inside expf), about 64 * 2^-24 = 4e-6
relative error of the mass each; expf itself adds a few ulp (~2e-7); truncation to 2^-40 fixed point loses at most 2^-40 per token, 2^-40 V <= 1e-6
of the top token's mass over a whole row.  A ratio of two such sums therefore differs from the float64 ratio by under 2e-5, and 1e-4 leaves about
5x on top.  The builders below place every threshold at least MARGIN away from its neighbours, so builder rows must match without exception.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

MARGIN = 1e-4
GAP = 2.02e-4  # the builders put p / u at the middle of a gap at least this wide (2e-4 and the float32 rounding of the threshold itself)
TORCH_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------------------------------
def is_greedy(t, p) -> bool:
    return bool(np.float32(t) < np.float32(1e-5) or np.float32(p) < np.float32(1e-8))


def process(logits_f32, t=1.0, r=1.0, history=()):
    """steps 1 and 2: x in np.float32, bit for bit what the kernel compares"""
    x = np.array(logits_f32, dtype=np.float32, copy=True)
    t, r = np.float32(t), np.float32(r)
    if t >= np.float32(1e-5) and t != np.float32(1.0):
        x = (x / t).astype(np.float32)
    if r > np.float32(1.0):
        ids = np.unique(np.asarray([h for h in history if 0 <= h < x.size], dtype=np.int64))
        if ids.size:
            xv = x[ids]
            x[ids] = np.where(xv < 0, xv * r, xv / r).astype(np.float32)
    return x


class Row:
    """the sorted structure of one processed row: masses, and per tie group (descending) the mass and the count above it"""

    def __init__(self, x):
        self.x = x
        self.V = x.size
        self.argmax = int(np.argmax(x))  # the lowest index among the maxima
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.exp(x.astype(np.float64) - np.float64(x.max()))
        self.m = np.where(np.isfinite(m), m, 0.0)
        self.Z = float(self.m.sum())
        vals, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)  # ascending; -0 and +0 are one value
        gm = np.bincount(inv.ravel(), weights=self.m, minlength=vals.size)[::-1]
        cnt = cnt[::-1]
        self.vals = vals[::-1]
        self.group_mass = gm / self.Z if self.Z > 0 else gm
        self.S_above = (np.cumsum(gm) - gm) / self.Z if self.Z > 0 else np.zeros_like(gm)
        self.N_above = np.cumsum(cnt) - cnt

    def kept(self, p=1.0, k=0):
        """steps 5 to 7 -> (mask of the kept tokens, the margin of p)"""
        p = np.float32(p)
        ok = np.ones(self.vals.size, dtype=bool)
        margin = np.inf
        if np.float32(1e-8) <= p < np.float32(1.0):
            ok &= self.S_above < np.float64(p)
            margin = float(np.min(np.abs(self.S_above - np.float64(p))))
        if 0 < k < self.V:
            ok &= self.N_above < k
        n = int(ok.sum())  # both conditions hold on a prefix of the descending groups; the top group always passes
        assert n >= 1 and ok[:n].all()
        return self.x >= self.vals[n - 1], margin

    def draw(self, mask, u):
        """step 8 for one or many u -> (tokens, margins of u)"""
        mk = np.where(mask, self.m, 0.0)
        C = np.cumsum(mk)
        Zk = C[-1]
        u = np.atleast_1d(np.asarray(u, dtype=np.float32)).astype(np.float64)
        target = u * Zk
        tok = np.searchsorted(C, target, side="right")  # the first v with C_v > u Zk: C only rises at kept tokens
        last = int(np.flatnonzero(mask)[-1])
        tok = np.where(tok >= self.V, last, tok)
        hi = C[tok]
        lo = np.where(tok > 0, C[np.maximum(tok - 1, 0)], 0.0)
        up = np.where(hi >= Zk, np.inf, (hi - target) / Zk)
        dn = np.where(lo <= 0.0, np.inf, (target - lo) / Zk)
        return tok.astype(np.int64), np.minimum(up, dn)


def sample_row(logits_f32, u, t=1.0, p=1.0, k=0, r=1.0, history=(), row=None):
    """the whole contract for one row -> (token, margin, kept mask or None for a greedy row)"""
    row = row if row is not None else Row(process(logits_f32, t, r, history))
    if is_greedy(t, p):
        return row.argmax, np.inf, None
    mask, mp = row.kept(p, k)
    tok, mu = row.draw(mask, u)
    return int(tok[0]), float(min(mp, mu[0])), mask


def advance(token, seqlen, max_len, stop_ids):
    """step 9 -> (new seqlen, finished)"""
    stop = token in set(stop_ids)
    return (-1 if stop or seqlen + 1 >= max_len else seqlen + 1), stop


# ------------------------------------------------------------------------------------------------------------------------
# builders: thresholds at the middle of wide gaps, so that every row is robust
# ------------------------------------------------------------------------------------------------------------------------
def make_logits(seed, rows, V, dtype_name):
    """N(0, 3.5) rounded to the dtype (ties then occur in bf16) -> (torch tensor [rows, V] of the dtype, the same values as np.float32)"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(rows, V, generator=g) * 3.5).to(TORCH_DTYPES[dtype_name])
    return t, t.float().numpy()


def place_p(row: Row, target: float) -> float:
    """p at the middle of the S-gap (= tie group) of width >= GAP whose middle is nearest to target"""
    mid = row.S_above + 0.5 * row.group_mass
    wide = np.flatnonzero(row.group_mass >= GAP)
    assert wide.size, "no tie group of probability >= GAP"
    g = wide[np.argmin(np.abs(mid[wide] - target))]
    p = float(np.float32(mid[g]))
    assert 1e-8 <= p < 1.0
    return p


def place_u(row: Row, mask, target: float) -> float:
    """u at the middle of the interval of the kept token of (renormalised) probability >= GAP whose middle is nearest to target"""
    mk = np.where(mask, row.m, 0.0)
    C = np.cumsum(mk)
    q = mk / C[-1]
    mid = C / C[-1] - 0.5 * q
    wide = np.flatnonzero(q >= GAP)
    assert wide.size, "no kept token of probability >= GAP"
    v = wide[np.argmin(np.abs(mid[wide] - target))]
    u = float(np.float32(mid[v]))
    assert 0.0 <= u < 1.0
    return u


# every vocabulary size the tests run: 1 and 7 (less than one 16-byte load), 1000 / 1023 / 1025 (rows that start off a 16-byte boundary, a tail),
# the vocabularies of Llama-2, Llama-3 and Qwen2, and the limit 2^20; all three dtypes at the small ones
SHAPES = tuple((V, ("fp32", "bf16", "fp16")) for V in (1, 7, 1000, 1023, 1025)) + tuple((V, ("bf16", "fp32")) for V in (32000, 128256, 151936, 1048576))
MODES = ("greedy_t", "greedy_p", "temperature", "plain", "topk1", "topk50", "topkV", "topp50", "topp95", "both_p_binds", "both_k_binds", "penalty",
         "penalty_len0")
HIST_LEN = 16


@functools.lru_cache(maxsize=None)
def build_case(V: int, dtype_name: str, seed: int = 0):
    """One row per mode of MODES over two random logit rows.  -> dict of per-row arrays: logits (torch, [M, V]), u, t, p, k, r (numpy), history
    [M, HIST_LEN], hist_len, and the oracle's token / margin per row."""
    lt, lf = make_logits(1000 * seed + V % 9973, 2, V, dtype_name)
    M = len(MODES)
    out = dict(u=np.zeros(M, np.float32), t=np.ones(M, np.float32), p=np.ones(M, np.float32), k=np.zeros(M, np.int32), r=np.ones(M, np.float32),
               history=np.zeros((M, HIST_LEN), np.int32), hist_len=np.zeros(M, np.int32), token=np.zeros(M, np.int64), margin=np.zeros(M),
               src=np.zeros(M, np.int64))
    rows = {}

    def stats(src, t, r, hist):
        key = (src, float(t), float(r), tuple(hist))
        if key not in rows:
            rows[key] = Row(process(lf[src], t, r, hist))
        return rows[key]

    top = np.resize(np.argsort(-lf[1], kind="stable")[:3], 3)
    hist = [int(top[0]), int(top[0]), int(top[1]), V + 5, -1, int(top[2]), int(top[0]), V, (7 * V) // 11, V // 2]  # repeats, ids outside [0, V)
    for i, mode in enumerate(MODES):
        src, t, r, h, k = i % 2, 0.7, 1.0, (), 0
        p_target = u_target = None
        if mode == "greedy_t":
            t, out["p"][i], k = 0.0, 0.9, 50
        elif mode == "greedy_p":
            out["p"][i] = 0.0
        elif mode == "temperature":
            u_target = 0.35
        elif mode == "plain":
            t, u_target = 1.0, 0.6
        elif mode == "topk1":
            k, u_target = 1, 0.5
        elif mode == "topk50":
            k, u_target = 50, 0.7
        elif mode == "topkV":
            k, u_target = V, 0.2
        elif mode == "topp50":
            p_target, u_target = 0.5, 0.8
        elif mode == "topp95":
            p_target, u_target = 0.95, 0.9
        elif mode == "both_p_binds":
            p_target, k, u_target = 0.5, max(V - 1, 1), 0.45
        elif mode == "both_k_binds":
            t, p_target, k, u_target = 1.5, 0.95, 3, 0.55  # (a flatter row: top-p 0.95 alone keeps far more than three)
        elif mode == "penalty":
            src, t, r, h, p_target, k, u_target = 1, 0.8, 1.3, tuple(hist), 0.9, 40, 0.1
        elif mode == "penalty_len0":
            src, t, r, h, u_target = 1, 0.8, 1.3, (), 0.65
        out["t"][i], out["r"][i], out["k"][i], out["src"][i] = t, r, k, src
        if mode.startswith("penalty"):
            out["history"][i, :len(hist)] = hist
            out["hist_len"][i] = len(h)
        row = stats(src, t, r, h)
        if p_target is not None:
            out["p"][i] = place_p(row, p_target)
        if u_target is None:
            out["u"][i] = 0.5
            out["token"][i], out["margin"][i] = row.argmax, np.inf
            continue
        mask, mp = row.kept(out["p"][i], k)
        if V >= 1000 and mode.startswith("both"):  # the named filter is the one that cuts
            by_p, by_k = int(row.kept(out["p"][i], 0)[0].sum()), int(row.kept(1.0, k)[0].sum())
            assert (by_p < by_k) == (mode == "both_p_binds") and by_p != by_k, (mode, by_p, by_k)
        out["u"][i] = place_u(row, mask, u_target)
        tok, mu = row.draw(mask, out["u"][i])
        out["token"][i], out["margin"][i] = tok[0], min(mp, mu[0])
    out["logits"] = lt[torch.from_numpy(out["src"])].contiguous()
    return out


@functools.lru_cache(maxsize=None)
def build_grid(N: int = 2048, V: int = 1000, k: int = 50, seed: int = 7):
    """One fp32 row repeated N times with u = (i + 0.5) / N and top-k -> (logits [V] torch, u [N], tokens [N], margins [N])"""
    lt, lf = make_logits(seed, 1, V, "fp32")
    row = Row(process(lf[0]))
    mask, _ = row.kept(1.0, k)
    u = ((np.arange(N) + 0.5) / N).astype(np.float32)
    tok, mu = row.draw(mask, u)
    return lt[0], u, tok, mu
