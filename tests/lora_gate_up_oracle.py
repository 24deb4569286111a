"""numpy restatement of the multi-LoRA expand on QuantLlamaMLP's gate / up pair (include/awq_cdna4.h: awq_lora_expand_gate_up; DESIGN.md "Multi-LoRA",
"The gate / up pair"), built on tests/lora_oracle.py (steps 1 - 4 of the LoRA contract) and tests/tail_oracle.py (the SiLU * mul tail).

The contract.  F = n2 / 2, slice 0 is gate, slice 1 is up.  y2 [total_q, 2F] is the base pair's output in the 8 + 8 interleaved column order
(columns 16 j .. 16 j + 7 gate rows 8 j .., columns 16 j + 8 .. 16 j + 15 the matching up rows); b_pool [S, 2F, R] holds B_gate's rows, then B_up's.
For every row t of an ACTIVE sequence b (1 <= Sq_b <= max_seqlen_q) and f < F, j = f / 8, c = f % 8:
  * with a valid a = adapter_ids[b]:  g' = T(f32(y2[t, 16 j + c]) + d_gate[t, f]),  u' = T(f32(y2[t, 16 j + 8 + c]) + d_up[t, f]) -- lora_oracle's steps
    1 - 4 on the de-interleaved pair [gate | up] with slice_end = (F, 2F);
  * without one:  g' = y2[t, 16 j + c],  u' = y2[t, 16 j + 8 + c], bit for bit;
  * h[t, f] = T(T(silu(g')) * u'): the library's silu runs on the hardware exp2 / rcp, so the CPU answer is tail_oracle's HULL -- two accepted
    codes per element (equal for most gates), not one.
Every other row (inactive or empty sequence, padding) keeps every bit of h, and its y2 is not read.

`accepted(case, mutant)` returns, per element of h, the two accepted codes (for rows that are not written: the sentinel, twice).  A result passes
when each element carries one of its two codes.  A MUTANT is rejected by a case when, on at least one element, its two codes are both different
from the target's two: then no tensor can pass both (tests/test_lora_gate_up_host.py asserts that for every mutant, on the CPU, so the GPU test
cannot pass a mutant)."""
import numpy as np
import torch

from tests import lora_oracle as L
from tests import tail_oracle as TO
from tests.lm_head_oracle import DTYPES, f64, round_T

PACKED_SQ, PACKED_IDS, PACKED_PAD = L.PACKED_SQ, L.PACKED_IDS, L.PACKED_PAD
PACKED = dict(sq=PACKED_SQ, ids=PACKED_IDS, pad=PACKED_PAD)

MUTANTS = ("slices_swapped", "partner_plus_16", "stacked_pairing", "gate_delta_dropped", "up_delta_dropped", "up_delta_after_mul", "gate_not_rounded",
           "no_adapter_rows_skipped", "no_adapter_reads_slot0", "padding_written", "b_rows_interleaved")

F_FORMS = (8, 24, 136)   # n2 = 16: one group; 48: groups that wrap the four waves unevenly; 272: one full 256-column tile plus a 16-column rest


def gpu_shapes(plan_fn=L.plan):
    """(K, R, F) of the GPU tests: every K in {64, 192, an uneven-split K}, every R and every F three times each, rotated as lora_oracle.gpu_shapes"""
    out = []
    for i, R in enumerate((16, 32, 64)):
        for j, kname in enumerate((64, 192, "uneven")):
            F = F_FORMS[(i + j) % 3]
            out.append((L.find_uneven_k(plan_fn, R, 2) if kname == "uneven" else kname, R, F))
    return out


# ---- the 8 + 8 interleave of the columns ----
def interleave(stacked):
    """[gate | up] [T, 2F] -> y2 [T, 2F] (any array or tensor type that has reshape)"""
    T_, N2 = stacked.shape
    F = N2 // 2
    g, u = stacked[:, :F].reshape(T_, F // 8, 1, 8), stacked[:, F:].reshape(T_, F // 8, 1, 8)
    cat = torch.cat if isinstance(stacked, torch.Tensor) else np.concatenate
    return cat([g, u], 2).reshape(T_, N2)


def deinterleave(y2):
    """y2 [T, 2F] -> [gate | up] [T, 2F]"""
    T_, N2 = y2.shape
    F = N2 // 2
    v = y2.reshape(T_, F // 8, 2, 8)
    cat = torch.cat if isinstance(y2, torch.Tensor) else np.concatenate
    return cat([v[:, :, 0, :].reshape(T_, F), v[:, :, 1, :].reshape(T_, F)], 1)


def _sentinel(total_q, n, dtype):
    sent = (0x3C00 + (np.arange(total_q)[:, None] * 37 + np.arange(n)[None, :] * 11) % 991).astype(np.int16)
    return torch.from_numpy(sent).view(dtype).clone()


def _finish(c, F):
    """a lora_oracle case over N = 2F with slice_end = (F, 2F) -> the gate / up case: y2 (NaN on the rows outside the contract), the sentinel of h,
    the masks of the rows"""
    T = DTYPES[c["dtype_name"]]
    own = L.owners(c["cu"], c["B"], c["total_q"], c["max_sq"])
    c["F"] = F
    c["active"] = own >= 0
    c["plain"] = c["active"] & (c["slot"] < 0)       # active rows without an adapter: the plain tail
    y2 = interleave(c["y_init"])
    y2[torch.from_numpy(~c["active"])] = float("nan")
    c["y2"] = y2.contiguous()
    c["h_init"] = _sentinel(c["total_q"], F, T)
    return c


def build_lattice(K, R, F, dtype_name, **kw):
    """lora_oracle.build_lattice's case (the packed step PACKED_SQ / PACKED_IDS / PACKED_PAD taken as is, or rect=) on the pair: N = 2F, slice_end =
    (F, 2F); y_init is the de-interleaved base pair [gate | up], y2 its interleaved form"""
    return _finish(L.build_lattice(K, R, 2 * F, (F, 2 * F), dtype_name, **kw), F)


def build_random(K, R, F, dtype_name, **kw):
    return _finish(L.build_random(K, R, 2 * F, (F, 2 * F), dtype_name, **kw), F)


# ---- g', u' ----
def _deltas(case, a_pool, b_pool):
    """steps 1 - 3 of the LoRA contract in float64: d [total_q, 2F] in [gate | up] order for the served rows (exact on the lattice), zeros elsewhere"""
    K, R, F, name = case["K"], case["R"], case["F"], case["dtype_name"]
    x = f64(case["x_store"])[:, :K]
    d = np.zeros((case["total_q"], 2 * F))
    sc = case["scaling"].numpy()
    for a in sorted(set(case["slot"][case["slot"] >= 0].tolist())):
        rows = np.nonzero(case["slot"] == a)[0]
        h = x[rows] @ a_pool[a].T
        hT = round_T((np.float32(sc[a]) * h.astype(np.float32)).astype(np.float64), name)
        for j in range(2):
            d[np.ix_(rows, np.arange(j * F, (j + 1) * F))] = hT[:, j * R:(j + 1) * R] @ b_pool[a, j * F:(j + 1) * F].T
    return d


def reference(case, mutant=None):
    """-> (g', u', written): float64 arrays [total_q, F] of T values and the bool mask of the rows of h the (mutant) contract writes.  The target:
    lora_oracle.reference on the de-interleaved pair with slice_end = (F, 2F), the plain pass-through on active rows without an adapter."""
    F, name, total_q = case["F"], case["dtype_name"], case["total_q"]
    y2 = f64(case["y2"])
    if mutant == "stacked_pairing":
        stacked = y2.copy()
    elif mutant == "partner_plus_16":      # the partner of column 16 j + c is taken 16 columns on: the next group's gate octet (the last group wraps)
        stacked = deinterleave(y2)
        stacked[:, F:] = np.roll(stacked[:, :F], -8, axis=1)
    else:
        stacked = deinterleave(y2)
    args = L.oracle_args(case)
    a_pool, b_pool = args["a_pool"].copy(), args["b_pool"].copy()
    R = case["R"]
    if mutant == "slices_swapped":
        a_pool = np.concatenate([a_pool[:, R:], a_pool[:, :R]], 1)
    if mutant == "gate_delta_dropped":
        b_pool[:, :F] = 0.0
    if mutant in ("up_delta_dropped", "up_delta_after_mul"):
        b_pool[:, F:] = 0.0
    if mutant == "b_rows_interleaved":
        b_pool = np.stack([deinterleave(b_pool[s].T).T for s in range(b_pool.shape[0])])      # row 16 j + c read for gate row 8 j + c
    args.update(a_pool=a_pool, b_pool=b_pool, y_init=np.nan_to_num(stacked), kplan=case.get("kplan"))      # (kplan: hand-sized cases below the kernel's K)
    # (no_adapter_reads_slot0: the x of a row without an adapter is NaN in the built cases, and the mutant reads it)
    y, _ = L.reference(mutant="no_adapter_slot0" if mutant == "no_adapter_reads_slot0" else None, **args)
    if mutant == "gate_not_rounded":      # the fp32 sum itself: exact in float64 on the lattice
        served = case["slot"] >= 0
        y[served, :F] = (np.nan_to_num(stacked) + _deltas(case, a_pool, b_pool))[served, :F]
    written = case["active"].copy()
    if mutant == "no_adapter_rows_skipped":
        written &= ~case["plain"]
    if mutant == "padding_written":
        written[:] = True
    out = np.where(written[:, None], y, np.nan)
    if mutant == "padding_written":      # what the kernel would read there
        out[~case["active"]] = stacked[~case["active"]]
    return out[:, :F], out[:, F:], written


NAN_CODE = -1      # every NaN pattern counts as one code


def _codes(t):
    b = TO.to_bits(t).astype(np.int64)
    return np.where(torch.isnan(t.float()).numpy(), NAN_CODE, b)


def _hull_of_values(x, dtype):
    """tail_oracle.silu_hull for gates that are float64 values rather than T values (the gate_not_rounded mutant)"""
    e, d = TO.silu64(x), TO.silu_delta(x)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = e * (1.0 - d), e * (1.0 + d)
    a, b = np.where((e == 0) | np.isinf(e), e, a), np.where((e == 0) | np.isinf(e), e, b)
    return TO.rne64_to_T(np.fmin(a, b), dtype), TO.rne64_to_T(np.fmax(a, b), dtype)


def accepted(case, mutant=None):
    """-> (lo, hi, written): int64 [total_q, F] accepted codes of h (bit patterns, NAN_CODE for NaN) -- tail_accept on the written rows, the
    sentinel's code twice on the others"""
    T = DTYPES[case["dtype_name"]]
    g, u, written = reference(case, mutant)
    gw, uw = np.where(written[:, None], g, 0.0), np.where(written[:, None], u, 0.0)
    uT = torch.from_numpy(uw).to(T)
    assert np.array_equal(f64(uT), uw, equal_nan=True)
    if mutant == "gate_not_rounded":
        lo, hi = _hull_of_values(gw, T)
        with np.errstate(invalid="ignore", over="ignore"):
            c_lo, c_hi = TO.rne64_to_T(f64(lo) * uw, T), TO.rne64_to_T(f64(hi) * uw, T)
    else:
        gT = torch.from_numpy(gw).to(T)
        assert np.array_equal(f64(gT), gw, equal_nan=True), "g' is not made of T values"
        c_lo, c_hi = TO.tail_accept(gT, uT)
    if mutant == "up_delta_after_mul":      # T(T(silu(g')) * up) first, up's delta added to the product afterwards
        args = L.oracle_args(case)
        d_up = _deltas(case, np.nan_to_num(args["a_pool"]), np.nan_to_num(args["b_pool"]))[:, case["F"]:]
        c_lo, c_hi = TO.rne64_to_T(f64(c_lo) + d_up, T), TO.rne64_to_T(f64(c_hi) + d_up, T)
    sent = _codes(case["h_init"])
    w = written[:, None]
    return np.where(w, _codes(c_lo), sent), np.where(w, _codes(c_hi), sent), written


def check(case, h, acc=None):
    """h (a T tensor [total_q, F]) against the accepted codes; returns the number of elements that took the upper code where the two differ"""
    lo, hi, _ = accepted(case) if acc is None else acc
    got = _codes(h.detach().cpu())
    bad = (got != lo) & (got != hi)
    assert not bad.any(), f"{int(bad.sum())} elements outside the accepted codes, first at {tuple(np.argwhere(bad)[0])}"
    return int(((got == hi) & (lo != hi)).sum())


def rejects(case, mutant, target=None):
    """True when the mutant's accepted codes are disjoint from the target's on at least one element"""
    t_lo, t_hi, _ = accepted(case) if target is None else target
    m_lo, m_hi, _ = accepted(case, mutant)
    return bool(((m_lo != t_lo) & (m_lo != t_hi) & (m_hi != t_lo) & (m_hi != t_hi)).any())
