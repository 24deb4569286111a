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


# Faults a kernel could plausibly have, each as a variation of the oracle: `mutant=name` on process / Row.kept / Row.draw / sample_row.  No kernel
# is ever built wrong: tests/test_sample_host.py proves on the CPU that the rows the GPU tests launch tell every one of them from the contract,
# with the margin on both sides, so a kernel with that fault would return the other token.
MUTANTS = {
    # the kept set (steps 5 to 7)
    "k+1": "top-k keeps k + 1 tokens",
    "k-1": "top-k keeps k - 1 tokens",
    "tie_cut_at_k": "the tie group that straddles k is cut by index so that exactly k tokens remain",
    "p_plus_group": "top-p keeps one tie group too many",
    "p_drop_crossing": "top-p drops the tie group that crosses p",
    "tau_low8": "tau's key with its low 8 bits cleared: the last select pass is skipped or mis-masked",
    "tau_low16": "tau's key with its low 16 bits cleared: the last two select passes",
    "neg_raw_order": "the keys of negative floats compare by their raw bits (the order among negatives reversed)",
    "minus_zero_below": "-0 is not folded onto +0 and orders below it",
    # the penalty (step 2)
    "pen_wrap": "history ids are taken mod V instead of being ignored outside [0, V)",
    "pen_per_occurrence": "the penalty is applied once per occurrence, not once per distinct id",
    "pen_always_div": "the penalty always divides (wrong for negative logits)",
    "pen_inverted": "the penalty's direction is inverted",
    "hist_len_ignored": "the whole history row is read, stale ids behind hist_len included",
    # the draw (step 8) and the greedy step (step 3)
    "no_renorm": "the draw compares with u Z instead of u Zk",
    "draw_sorted": "the CDF runs in descending-mass order instead of index order",
    "greedy_ignores_penalty": "the greedy token is taken before the penalty",
    "greedy_highest_index": "the greedy token is the highest index among the maxima",
}
PROCESS_MUTANTS = ("pen_wrap", "pen_per_occurrence", "pen_always_div", "pen_inverted", "hist_len_ignored")


def key_of(x, fold=True, flip_neg=True):
    """the kernel's monotone float -> unsigned key (sample_key); fold / flip_neg off give the keys of two mutants"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float32))
    b = x.view(np.uint32).copy()
    if fold:
        b[x == 0] = 0
    neg = (b >> np.uint32(31)).astype(bool)
    return np.where(neg & flip_neg, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def process(logits_f32, t=1.0, r=1.0, history=(), mutant=None, stale=()):
    """steps 1 and 2: x in np.float32, bit for bit what the kernel compares (stale: the history row behind hist_len, which only a mutant reads)"""
    x = np.array(logits_f32, dtype=np.float32, copy=True)
    t, r = np.float32(t), np.float32(r)
    if t >= np.float32(1e-5) and t != np.float32(1.0):
        x = (x / t).astype(np.float32)
    if r > np.float32(1.0):
        history = [int(h) for h in history] + ([int(h) for h in stale] if mutant == "hist_len_ignored" else [])
        if mutant == "pen_wrap":
            history = [h % x.size for h in history]
        ids = np.asarray([h for h in history if 0 <= h < x.size], dtype=np.int64)
        for v in (ids if mutant == "pen_per_occurrence" else np.unique(ids)):
            if mutant == "pen_always_div":
                x[v] = x[v] / r
            elif mutant == "pen_inverted":
                x[v] = x[v] / r if x[v] < 0 else x[v] * r
            else:
                x[v] = x[v] * r if x[v] < 0 else x[v] / r
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
        self.vals, self.group_mass, self.S_above, self.N_above = self._groups(x)  # (-0 and +0 are one value)

    def _groups(self, order):
        """tie groups under `order` (the values themselves, or a mutant's keys), descending -> (values, mass, mass above, count above)"""
        vals, inv, cnt = np.unique(order, return_inverse=True, return_counts=True)
        gm = np.bincount(inv.ravel(), weights=self.m, minlength=vals.size)[::-1]
        cnt = cnt[::-1]
        Z = self.Z if self.Z > 0 else 1.0
        return vals[::-1], gm / Z, (np.cumsum(gm) - gm) / Z, np.cumsum(cnt) - cnt

    def kept(self, p=1.0, k=0, mutant=None):
        """steps 5 to 7 -> (mask of the kept tokens, the margin of p)"""
        p = np.float32(p)
        use_p, use_k = bool(np.float32(1e-8) <= p < np.float32(1.0)), 0 < k < self.V
        order, groups = self.x, (self.vals, self.group_mass, self.S_above, self.N_above)
        if mutant in ("neg_raw_order", "minus_zero_below"):
            order = key_of(self.x, fold=mutant != "minus_zero_below", flip_neg=mutant != "neg_raw_order").astype(np.int64)
            groups = self._groups(order)
        vals, group_mass, S_above, N_above = groups
        ok = np.ones(vals.size, dtype=bool)
        margin = np.inf
        if use_p:
            edges = S_above
            okp = S_above < np.float64(p)
            if mutant == "p_plus_group":
                okp[min(int(okp.sum()), okp.size - 1)] = True
            elif mutant == "p_drop_crossing":
                edges = S_above + group_mass
                okp = edges <= np.float64(p)
                okp[0] = True
            ok &= okp
            margin = float(np.min(np.abs(edges - np.float64(p))))
        if use_k:
            ok &= N_above < (k + 1 if mutant == "k+1" else max(k - 1, 1) if mutant == "k-1" else k)
        n = int(ok.sum())  # both conditions hold on a prefix of the descending groups; the top group always passes
        assert n >= 1 and ok[:n].all()
        mask = order >= vals[n - 1]
        if mutant in ("tau_low8", "tau_low16") and (use_p or use_k):
            tau = key_of(vals[n - 1])[0] & np.uint32(0xFFFFFF00 if mutant == "tau_low8" else 0xFFFF0000)
            mask = key_of(self.x) >= tau
        if mutant == "tie_cut_at_k" and use_k and int(mask.sum()) > k:
            mask = mask.copy()
            mask[np.flatnonzero(order == vals[n - 1])[k - int(mask.sum()):]] = False
        return mask, margin

    def draw(self, mask, u, mutant=None):
        """step 8 for one or many u -> (tokens, margins of u)"""
        mk = np.where(mask, self.m, 0.0)
        idx = np.argsort(-mk, kind="stable") if mutant == "draw_sorted" else np.arange(self.V)
        C = np.cumsum(mk[idx])
        Zk = C[-1]
        u = np.atleast_1d(np.asarray(u, dtype=np.float32)).astype(np.float64)
        target = u * (self.Z if mutant == "no_renorm" else Zk)
        tok = np.searchsorted(C, target, side="right")  # the first v with C_v > u Zk: C only rises at kept tokens
        last = int(np.flatnonzero(mask[idx])[-1])
        tok = np.where(tok >= self.V, last, tok)
        hi = C[tok]
        lo = np.where(tok > 0, C[np.maximum(tok - 1, 0)], 0.0)
        up = np.where(hi >= Zk, np.inf, (hi - target) / Zk)
        dn = np.where(lo <= 0.0, np.inf, (target - lo) / Zk)
        return idx[tok].astype(np.int64), np.minimum(up, dn)


def sample_rows(logits_f32, u, t=1.0, p=1.0, k=0, r=1.0, history=(), row=None, mutant=None, stale=()):
    """the whole contract for one row under one or many u -> (tokens, margins, kept mask or None for a greedy row).  `row`: the Row of the
    processed logits if the caller has it already (not used under a mutant of `process`)."""
    assert mutant is None or mutant in MUTANTS, mutant
    if row is None or mutant in PROCESS_MUTANTS:
        row = Row(process(logits_f32, t, r, history, mutant, stale))
    u = np.atleast_1d(np.asarray(u, dtype=np.float32))
    if is_greedy(t, p):
        tok = row.argmax
        if mutant == "greedy_ignores_penalty":
            tok = int(np.argmax(process(logits_f32, t)))
        elif mutant == "greedy_highest_index":
            tok = row.V - 1 - int(np.argmax(row.x[::-1]))
        return np.full(u.size, tok, np.int64), np.full(u.size, np.inf), None
    mask, mp = row.kept(p, k, mutant)
    tok, mu = row.draw(mask, u, mutant)
    return tok, np.minimum(mu, mp), mask


def sample_row(logits_f32, u, t=1.0, p=1.0, k=0, r=1.0, history=(), row=None, mutant=None, stale=()):
    """the whole contract for one row -> (token, margin, kept mask or None for a greedy row)"""
    tok, margin, mask = sample_rows(logits_f32, u, t, p, k, r, history, row, mutant, stale)
    return int(tok[0]), float(margin[0]), mask


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


# ------------------------------------------------------------------------------------------------------------------------
# edge rows: flat heads whose kept set decides the token (build_case's rows are peaked: a kept set off by one token moves their CDF by less than
# half the interval u sits in), each under a grid of u.  Same margin rule as above: every row keeps MARGIN, none is excluded.
# ------------------------------------------------------------------------------------------------------------------------
# 13: less than two chunks; 1000 / 1025: one pass iteration, a scalar tail; 40965 = 32768 + 8192 + 5: the max and select passes start a second
# iteration with a partly filled unroll group, a lane of the tile-sum scan owns two tiles, and the rows behind the first start off a boundary
EDGE_SHAPES = tuple((V, d) for V in (13, 1000, 1025, 40965) for d in ("fp32", "bf16", "fp16"))
U_GRID = 64                                          # u = (i + 0.5) / 64, then the two ends: 0 and 1 - 2^-24
LADDER_STEPS = (0, 1, 2, 3, 4, 5, 6, 6, 6, 7, 8, 9)  # head value by rank, in steps of 2^-5 below the top: ranks 7, 8, 9 (from 1) are one tie group
DENSE_OFF = 37                                       # tau of a dense row sits this many values off the middle: its low key byte is not 0


def head_indices(V):
    """where the ladder's twelve head tokens sit: the row's ends, either side of the chunk (8), tile (512) and pass-iteration (32768) borders, the
    scalar tail chunk -> ascending indices"""
    out = []
    for c in (0, V - 1, 7, 8, 63, 64, 511, 512, 513, 32767, 32768, V - 3, 255, 256, 1, 2, 3, 4, 5, 6, 9, 10):
        if 0 <= c < V and c not in out and len(out) < len(LADDER_STEPS):
            out.append(c)
    return sorted(out)


def head_ids(V):
    """the head's token ids by rank (0 = the largest logit); the rank of the j-th head index is (5 j + 3) % 12, so index order is not mass order"""
    idx = head_indices(V)
    by_rank = [0] * len(idx)
    for j, v in enumerate(idx):
        by_rank[(5 * j + 3) % len(idx)] = v
    return by_rank


def tail_logits(V):
    """-22 ... -23.875 in steps of 1/8 (exact in every dtype): under 1e-4 of the mass of any head below, whole"""
    return (-22.0 - (np.arange(V) % 16) / 8.0).astype(np.float32)


def ladder_logits(V, top):
    x = tail_logits(V)
    for rank, v in enumerate(head_ids(V)):
        x[v] = top - LADDER_STEPS[rank] / 32.0
    return x


def ladder_history(V):
    """-> (history row, hist_len): the top id twice, ids outside [0, V) that wrap onto head ids, and stale head ids behind hist_len"""
    h = head_ids(V)
    hist = np.zeros(HIST_LEN, np.int32)
    hist[:7] = [h[0], h[0], V + h[2], -1, h[4] - V, h[1], h[3]]
    return hist, 5


def _from_bits(bits, dtype_name):
    """consecutive bit patterns of the dtype -> their values as np.float32"""
    bits = np.asarray(bits, dtype=np.int64)
    if dtype_name == "fp32":
        return bits.astype(np.uint32).view(np.float32)
    if dtype_name == "bf16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.astype(np.uint16).view(np.float16).astype(np.float32)


def dense_logits(V, dtype_name, around):
    """A run of consecutive representable values of the dtype around 1.0 / -1.0 / across +-0 (both zeros and the denormals either side), scattered
    over the row; the rest is tail.  600 values; bf16 around +-1: 256, one binade either side (600 would span e^7 in mass).
    -> (x, k): top-k k puts tau DENSE_OFF values off the middle of the run"""
    one, sign = {"fp32": (0x3F800000, 0x80000000), "bf16": (0x3F80, 0x8000), "fp16": (0x3C00, 0x8000)}[dtype_name]
    half = 128 if dtype_name == "bf16" and around != "0" else 300
    j = np.arange(-half, half)
    if around == "p1":
        vals, tau = _from_bits(one + j, dtype_name), _from_bits([one - DENSE_OFF], dtype_name)[0]
    elif around == "m1":
        vals, tau = _from_bits(sign + one + j, dtype_name), _from_bits([sign + one + DENSE_OFF], dtype_name)[0]
    else:
        vals, tau = _from_bits(np.where(j >= 0, j, sign - 1 - j), dtype_name), _from_bits([sign + DENSE_OFF], dtype_name)[0]
    rng = np.random.default_rng(V + len(around))
    x = tail_logits(V)
    x[rng.permutation(V)[:vals.size]] = vals[rng.permutation(vals.size)]
    return x, int((x >= tau).sum())


def zero_logits(V):
    """the top group is -0, +0, -0, +0 (the lowest index holds a -0); three tokens at -0.5 below it; the rest is tail"""
    x = tail_logits(V)
    x[[2, V - 1]], x[[5, 8]] = [-0.0, 0.0], [0.0, -0.0]
    x[[0, 6, V - 2]] = -0.5
    return x


def robust_u(row: Row, mask, u):
    """u, or where u is within the margin of a boundary, the middle of the interval it fell in (of a wide interval nearby where that one is thin)"""
    tok, margin = row.draw(mask, u)
    if margin[0] >= GAP / 2:
        return float(u)
    mk = np.where(mask, row.m, 0.0)
    C = np.cumsum(mk)
    if mk[tok[0]] / C[-1] >= GAP:
        return float(np.float32((C[tok[0]] - 0.5 * mk[tok[0]]) / C[-1]))
    return place_u(row, mask, float(u))


def edge_grid(row: Row, mask):
    u = [robust_u(row, mask, np.float32((i + 0.5) / U_GRID)) for i in range(U_GRID)] + [0.0, 1.0 - 2.0 ** -24]  # (the ends stay where they are)
    return np.asarray(u, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def build_edge_case(V: int, dtype_name: str):
    """The edge configurations of one (V, dtype): -> a tuple of dicts, one per configuration = one logits row (x: np.float32, logits: torch of the
    dtype) with its parameters, history and U_GRID + 2 uniforms, and the oracle's token / margin per uniform.  `family` names what the row is
    (ladder+, ladder-, dense, zero)."""
    out = []

    def add(name, family, x, t=1.0, p_target=None, k=0, r=1.0, hist=None):
        lt = torch.from_numpy(x).to(TORCH_DTYPES[dtype_name])
        assert np.array_equal(lt.float().numpy().view(np.uint32), x.view(np.uint32)), name      # the values are exact in the dtype
        history, hist_len = hist if hist is not None else (np.zeros(HIST_LEN, np.int32), 0)
        row = Row(process(x, t, r, history[:hist_len]))
        p = place_p(row, p_target) if p_target is not None and p_target > 0 else (0.0 if p_target == 0 else 1.0)
        c = dict(name=name, family=family, V=V, dtype=dtype_name, x=x, logits=lt, t=np.float32(t), p=np.float32(p), k=int(k), r=np.float32(r),
                 history=history, hist_len=hist_len, row=row)
        c["u"] = np.full(U_GRID + 2, 0.5, np.float32) if is_greedy(t, p) else edge_grid(row, row.kept(p, k)[0])
        c["token"], c["margin"] = edge_tokens(c)
        out.append(c)

    for sign, top in (("+", 2.0), ("-", -1.0)):
        x, hist, fam = ladder_logits(V, top), ladder_history(V), "ladder" + sign
        add(f"ladder{sign}_topk8_tie", fam, x, k=8)
        add(f"ladder{sign}_topk5_t0.7", fam, x, t=0.7, k=5)
        add(f"ladder{sign}_topp", fam, x, p_target=0.5)
        add(f"ladder{sign}_pen1.3", fam, x, r=1.3, hist=hist)
        add(f"ladder{sign}_pen1.5_k6_p0.8_t0.9", fam, x, t=0.9, p_target=0.8, k=6, r=1.5, hist=hist)
        add(f"ladder{sign}_greedy_pen1.3", fam, x, t=0.0, r=1.3, hist=hist)
    if V >= 1000:
        for around in ("p1", "m1", "0"):
            x, k = dense_logits(V, dtype_name, around)
            add(f"dense_{around}", "dense", x, t=1.0 if dtype_name == "fp32" else 0.7, k=k)   # (16-bit values: the division fills the low key bits)
    add("zero_topk2", "zero", zero_logits(V), t=0.7, k=2)
    add("zero_greedy", "zero", zero_logits(V), p_target=0)
    return tuple(out)


def edge_tokens(c, mutant=None, u=None):
    """the tokens and margins of one edge configuration under its own uniforms (or u), by the contract or by a mutant of it"""
    h, n = c["history"], c["hist_len"]
    tok, margin, _ = sample_rows(c["x"], c["u"] if u is None else u, c["t"], c["p"], c["k"], c["r"], h[:n], c["row"], mutant, h[n:])
    return tok, margin


def can_express(mutant, family, dtype_name):
    """Whether a row family can tell the mutant from the contract at all.  The orderings of negative keys and of -0 need tau among such keys; a
    cleared low byte (two bytes) of tau's key takes in another token only where keys lie closer than 2^8 (2^16): consecutive fp32 values, and
    for 2^16 consecutive fp16 values (2^13 apart as fp32 keys) -- bf16 values are 2^16 apart, so no bf16 row can show either."""
    if mutant == "tau_low8":
        return family == "dense" and dtype_name == "fp32"
    if mutant == "tau_low16":
        return family == "dense" and dtype_name in ("fp32", "fp16")
    if mutant == "neg_raw_order":
        return family in ("ladder-", "dense")
    if mutant == "minus_zero_below":
        return family == "zero"
    if mutant == "greedy_highest_index":
        return family == "zero"
    return family.startswith("ladder")
