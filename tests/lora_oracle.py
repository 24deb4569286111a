"""numpy restatement of the multi-LoRA contract (include/awq_cdna4.h: awq_lora_shrink, awq_lora_expand; DESIGN.md "Multi-LoRA") in float64, the
builders of the test cases, the mutants and the per-element bound.

The contract, for every packed row t owned by an ACTIVE sequence b (1 <= Sq_b <= max_seqlen_q) whose a = adapter_ids[b] lies in [0, S)
(T = bf16 or fp16; the owner of t is the LAST b with cu[b] <= t < cu[b + 1], rows >= cu[B] are padding; without cu_seqlens_q sequence b owns rows
b * max_seqlen_q .. (b + 1) * max_seqlen_q - 1):
  1. h32[t, c] = sum_k f32(x[t, k]) * f32(A_a[c, k]) in fp32, c < RS = n_slices * R; the k range is cut into KS splits (`plan`), the partial of split
     s goes to ws[s, t, c].
  2. hT[t, c] = T(scaling[a] * (ws[0, t, c] + ws[1, t, c] + ...)): one fp32 product, one nearest-even rounding to T.
  3. d32[t, n] = sum_{r < R} f32(hT[t, j(n) * R + r]) * f32(B_a[n, r]) in fp32, j(n) = the slice of column n.
  4. y[t, n] = T(f32(y[t, n]) + d32[t, n]): one rounding; the delta is not rounded to T before the add.
Every other row keeps every bit of y.

Two ways to hold a result to this.

LATTICE cases (`build_lattice`): x, A, B, y are small integers times powers of two and scaling is m * 2^e with m = 1 (or m = 3: the family whose
product in step 2 is not a power-of-two shift).  The builder ASSERTS sum |x||a| < 2^24, sum |hT||b| < 2^24 and |y| + |d| < 2^24 lattice units, so
every fp32 sum is exact in any order, the product of step 2 is exact in fp32 (emulated with np.float32 all the same), and the two roundings to T
are the only roundings: `reference(.., ideal=False)` reproduces them and the expected BITS are exact -- bound zero.  hT is an integer number of
lattice units whatever it rounds to, because rounding an integer to fewer bits gives an integer.  The builder moves two h values and two final y
values onto ties of T, one that rounds up and one that rounds down.

RANDOM cases (`build_random`): `reference(.., ideal=True)` returns the real-number value y* = y + sum_r (scaling * h)[r] * B[n, r] with NO rounding,
and `bound` the derived distance the contract may keep from it (derived, not measured).  A product of two T values has at most 22 significant bits
and is exact in fp32.  A sum of K exact terms taken in any order with one rounding per addition (u = 2^-24) errs by at most (K - 1) u sum |x a|
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the (1 + u)^K slack is below 1e-3 of the bound for K <= 16384); the product
with scaling is one more rounding, and K + 1 is used where K would do:
      e_h  = |scaling| * (K + 1) * 2^-24 * sum_k |x a|  +  ulp_T(|scaling * h| + that) / 2          the fp32 sum and product, then half an ulp of T for hT
      e_d  = sum_r e_h[r] |B[n, r]|  +  (R + 1) * 2^-24 * (sum_r (|scaling * h|[r] + e_h[r]) |B[n, r]| + |y|)    e_h propagated; the second sum and the add of y
      |y_T - y*| <= e_d + ulp_T(|y*| + e_d) / 2                                                      half an ulp of T of the result
The matrix unit adds 32 products per instruction to an fp32 accumulator; any grouping is covered by "any order", and fewer roundings than one per
term only lower the error.  The K split changes the order of the sum, not the number of terms.

MUTANTS are one-line deviations of `reference`.  Every one changes the expected bits of at least one lattice case (tests/test_lora_host.py); those
that are not roundings (`ROUNDING_MUTANTS`) also leave the bound of a random case.
"""
import numpy as np
import torch

from tests.lm_head_oracle import DTYPES, PREC, f64, round_T, ulp_T

K_STEP = 64
ROW_TILE = 16
MUTANTS = ("tile_first_adapter", "ids_ignored", "no_adapter_slot0", "owner_first", "scaling_dropped", "scale_after_round", "h_unrounded",
           "delta_rounded", "split0_only", "last_split_dropped", "r16_only", "slice0_h", "row_prev", "ldx_as_k", "padding_written", "trunc")
ROUNDING_MUTANTS = ("scale_after_round", "h_unrounded", "delta_rounded", "trunc")   # below the random bound by design: the lattice is what sees them

# the packed step of the issue: a valid id on an empty sequence (2), an out-of-range id on a live one (7), a run of empty sequences in front of a
# live one (1, 2 -> 3), a sequence of exactly one tile (5), one of two tiles and a row (6), and a 16-row global tile shared by several adapters
PACKED_SQ = (1, 0, 0, 17, 3, 16, 33, 1)
PACKED_IDS = (0, -1, 2, 1, 0, 2, 1, 3)   # S = 3: the last id is out of range
PACKED_PAD = 4


def plan(K, R, n_slices):
    """awq_lora_plan restated: (KS, k per split).  About 64 KiB of A per shrink block, whole 64-k steps, at least four steps (one per wave), at most
    32 splits, dealt evenly; split s sums k in [s * kper, min(K, (s + 1) * kper))."""
    rs, steps = R * n_slices, K // K_STEP
    per = max(4, 65536 // (2 * rs) // K_STEP)
    ks = min(32, -(-steps // per))
    per = -(-steps // ks)
    ks = -(-steps // per)
    return ks, per * K_STEP


def find_uneven_k(plan_fn, R, n_slices):
    """the smallest K whose plan has KS >= 2 splits with different numbers of 64-k steps"""
    for steps in range(2, 4096):
        ks, kper = plan_fn(steps * K_STEP, R, n_slices)
        if ks >= 2 and steps % ks != 0:
            return steps * K_STEP
    raise AssertionError("no K found")


N_FORMS = ((16, (16,)), (48, (48,)), (80, (48, 64, 80)))   # (N, slice_end)


def gpu_shapes(plan_fn=plan):
    """(K, R, N, slice_end) of the GPU tests: every K in {64, 192, an uneven-split K}, every R and every N form at least three times each"""
    out = []
    for i, R in enumerate((16, 32, 64)):
        for j, kname in enumerate((64, 192, "uneven")):
            N, ends = N_FORMS[(i + j) % 3]
            K = find_uneven_k(plan_fn, R, len(ends)) if kname == "uneven" else kname
            out.append((K, R, N, ends))
    return out


def owners(cu, B, total_q, max_sq, mutant=None):
    """per packed row: the owning sequence if it is active, else -1"""
    own = np.full(total_q, -1, dtype=np.int64)
    if cu is None:
        for b in range(B):
            own[b * max_sq:(b + 1) * max_sq] = b
        return own
    cu = [int(c) for c in cu]
    for t in range(min(cu[B], total_q)):
        top = max(cu[b] for b in range(B) if cu[b] <= t)
        cand = [b for b in range(B) if cu[b] == top]
        b = cand[0] if mutant == "owner_first" else cand[-1]
        if 1 <= cu[b + 1] - cu[b] <= max_sq:
            own[t] = b
    return own


def row_slots(ids, cu, B, total_q, max_sq, S, mutant=None):
    """per packed row: the slot that serves it, -1 = the row keeps its y"""
    own = owners(cu, B, total_q, max_sq, mutant)
    slot = np.full(total_q, -1, dtype=np.int64)
    for t in range(total_q):
        if own[t] < 0:
            continue
        a = int(ids[own[t]])
        if mutant == "ids_ignored":
            a = 0
        if mutant == "no_adapter_slot0" and not 0 <= a < S:
            a = 0
        slot[t] = a if 0 <= a < S else -1
    if mutant == "tile_first_adapter":
        for t in range(total_q):
            t0 = t // ROW_TILE * ROW_TILE
            if slot[t] >= 0 and slot[t0] >= 0:
                slot[t] = slot[t0]
    if mutant == "padding_written" and cu is not None and (slot >= 0).any():
        slot[int(cu[B]):] = slot[slot >= 0][-1]
    return slot


def slice_of(n, slice_end):
    return int(np.searchsorted(np.asarray(slice_end), n, side="right"))


def reference(x_store, ldx, total_q, a_pool, b_pool, scaling, ids, cu, max_sq, slice_end, y_init, dtype_name, ideal=False, mutant=None, kplan=None):
    """steps 1 - 4 in float64.  x_store: float64 array, the storage of x (row t at t * ldx); a_pool [S, RS, K], b_pool [S, N, R], y_init [total_q, N]
    float64 arrays of T values; scaling: np.float32 [S]; ids / cu: integer arrays (cu None = rectangular).  ideal=False: the two roundings to T are
    taken (exact on the lattice); ideal=True: none is, and the second result is the docstring's bound.  Returns (y [total_q, N], bound or None)."""
    S, RS, K = a_pool.shape
    N, R = b_pool.shape[1:]
    B = len(ids)
    ks, kper = kplan if kplan is not None else plan(K, R, len(slice_end))
    flat = np.asarray(x_store, dtype=np.float64).reshape(-1)
    lx = K if mutant == "ldx_as_k" else ldx
    x = np.stack([flat[t * lx: t * lx + K] for t in range(total_q)])
    if mutant == "row_prev":
        x = np.concatenate([x[:1], x[:-1]])
    slot = row_slots(ids, cu, B, total_q, max_sq, S, mutant)
    kk = kper if mutant == "split0_only" else ((ks - 1) * kper if mutant == "last_split_dropped" and ks > 1 else K)
    rr = 16 if mutant == "r16_only" else R
    trunc = mutant == "trunc"
    y = np.array(y_init, dtype=np.float64)
    bnd = np.zeros_like(y) if ideal else None
    ends = [0] + list(slice_end)
    for a in sorted(set(slot[slot >= 0].tolist())):
        rows = np.nonzero(slot == a)[0]
        A, Bm, sc = a_pool[a], b_pool[a], np.float32(scaling[a])
        with np.errstate(invalid="ignore", over="ignore"):
            h = x[rows][:, :kk] @ A[:, :kk].T
            absxa = np.abs(x[rows]) @ np.abs(A).T
            if ideal:
                hs = h if mutant == "scaling_dropped" else float(sc) * h
                hT = hs
                e_h = abs(float(sc)) * (K + 1) * 2.0 ** -24 * absxa
                e_h = e_h + ulp_T(np.abs(hs) + e_h, dtype_name) / 2
            else:
                if mutant == "scaling_dropped":
                    hs = h
                elif mutant == "scale_after_round":
                    hs = h
                else:
                    hs = (sc * h.astype(np.float32)).astype(np.float64)     # one fp32 product (h is exact in fp32 on the lattice)
                hT = hs if mutant == "h_unrounded" else np.where(np.isfinite(hs), round_T(np.nan_to_num(hs), dtype_name, truncate=trunc), hs)
                if mutant == "scale_after_round":
                    hT = hT * float(sc)
            d = np.zeros((len(rows), N))
            e_d = np.zeros((len(rows), N))
            for j in range(len(slice_end)):
                lo, hi = ends[j], ends[j + 1]
                jj = 0 if mutant == "slice0_h" else j
                hj = hT[:, jj * R: jj * R + rr]
                d[:, lo:hi] = hj @ Bm[lo:hi, :rr].T
                if ideal:
                    ej = e_h[:, jj * R: jj * R + rr]
                    absB = np.abs(Bm[lo:hi, :rr]).T
                    e_d[:, lo:hi] = ej @ absB + (R + 1) * 2.0 ** -24 * ((np.abs(hj) + ej) @ absB + np.abs(y[rows][:, lo:hi]))
            if mutant == "delta_rounded":
                d = np.where(np.isfinite(d), round_T(np.nan_to_num(d), dtype_name), d)
            s = y[rows] + d
            if ideal:
                y[rows] = s
                bnd[rows] = e_d + ulp_T(np.abs(s) + e_d, dtype_name) / 2
            else:
                y[rows] = np.where(np.isfinite(s), round_T(np.nan_to_num(s), dtype_name, truncate=trunc), s)
    return y, bnd


# ---- builders ----

def tie_direction(s, dtype_name):
    """'up' / 'down' if |s| (an integer number of lattice units that T holds up to 2^p exactly) lies half way between two T values, else None"""
    p = PREC[dtype_name]
    a = abs(int(s))
    if a < 2 ** p:
        return None
    ulp = 2 ** (a.bit_length() - p)
    if a % ulp != ulp // 2:
        return None
    return "up" if (a // ulp) % 2 == 1 else "down"


def _tie_targets(dtype_name, m):
    """two integers v = m * h (h integer) on ties of T, the first rounding up, the second down, a little above 2^(p + 1)"""
    out = {}
    v = 2 ** (PREC[dtype_name] + 1)
    while len(out) < 2:
        v += 1
        d = tie_direction(v, dtype_name)
        if d is not None and v % m == 0 and d not in out:
            out[d] = v
    return out["up"], out["down"]


def _t_integers(dtype_name):
    """the integers of magnitude below 2^(p + 5) that T holds exactly"""
    p = PREC[dtype_name]
    vals = set()
    for j in range(6):
        for m in range(2 ** p):
            vals.add(m << j)
    pos = np.array(sorted(vals), dtype=np.int64)
    return np.concatenate([-pos[:0:-1], pos])


def layout(sq, pad):
    cu = np.concatenate([[0], np.cumsum(sq)]).astype(np.int32)
    return cu, int(cu[-1]) + pad


def build_lattice(K, R, N, slice_end, dtype_name, sq=None, ids=None, pad=0, rect=None, S=3, scale_m=1, max_sq=None, seed=0):
    """A lattice case.  sq / ids / pad: a packed step (cu_seqlens_q is built); rect = (B, rows per sequence): the rectangular form (ids default to
    b % S).  x has ldx = K + 8 with NaN in the gap, NaN in the rows of padding and of sequences without an adapter; pool slots that no served row
    names are NaN; y rows that must survive hold a sentinel pattern.  Returns a dict of torch tensors (CPU), numpy ids / cu, and `expected` (T)."""
    rng = np.random.default_rng(seed + 7 * K + 13 * N + 17 * R + (500 if dtype_name == "fp16" else 0) + 3 * scale_m)
    T = DTYPES[dtype_name]
    ns = len(slice_end)
    RS = R * ns
    if rect is not None:
        B, rows = rect
        cu, total_q, max_sq = None, B * rows, rows
        ids = np.array([b % S for b in range(B)] if ids is None else ids, dtype=np.int32)
    else:
        cu, total_q = layout(sq, pad)
        B = len(sq)
        ids = np.array(ids, dtype=np.int32)
        max_sq = max(sq) if max_sq is None else max_sq
    slot = row_slots(ids, cu, B, total_q, max_sq, S)
    served = np.nonzero(slot >= 0)[0]
    assert len(served) > 0
    used = sorted(set(slot[served].tolist()))
    EX, EA, EB = -2, -4, -3
    xi = rng.integers(-7, 8, size=(total_q, K)).astype(np.float64)
    ai = rng.integers(-15, 16, size=(S, RS, K)).astype(np.float64)
    bi = rng.integers(-3, 4, size=(S, N, R)).astype(np.float64)
    sc_e = np.array([-1, 1, -2, 2, -3][:S] if S <= 5 else rng.integers(-3, 3, S), dtype=np.float64)
    scaling = (scale_m * 2.0 ** sc_e).astype(np.float32)
    # two h values on ties: row t0 = the first served row, columns 0 and 1 of its adapter, through x[t0, 0] = 64, x[t0, 1] = 1
    t0 = int(served[0])
    a0 = int(slot[t0])
    xi[t0, 0], xi[t0, 1] = 64.0, 1.0
    h_ties = []
    for c, target in zip((0, 1), _tie_targets(dtype_name, scale_m)):
        s = float(xi[t0] @ ai[a0, c])
        dlt = target // scale_m - s
        q = int(np.rint(dlt / 64.0))
        r = int(dlt - 64 * q)
        if abs(ai[a0, c, 0] + q) <= 255 and abs(ai[a0, c, 1] + r) <= 255:      # eight significant bits: a T value in both formats
            ai[a0, c, 0] += q
            ai[a0, c, 1] += r
            h_ties.append(c)
    assert len(h_ties) == 2, "the h ties could not be placed"
    # exactness of steps 1 and 2
    for a in used:
        rows = np.nonzero(slot == a)[0]
        assert (np.abs(xi[rows]) @ np.abs(ai[a]).T).max() < 2 ** 24, "not a lattice case: a partial sum of h could round"
        assert (np.abs(xi[rows] @ ai[a].T) * scale_m).max() < 2 ** 24, "not a lattice case: scaling * h is not exact in fp32"
    x_unit, a_unit, b_unit = 2.0 ** EX, 2.0 ** EA, 2.0 ** EB
    ldx = K + 8
    x_store = torch.full((total_q, ldx), float("nan"), dtype=T)
    x_store[served, :K] = torch.from_numpy(xi[served] * x_unit).to(T)
    a_pool = torch.full((S, RS, K), float("nan"), dtype=T)
    b_pool = torch.full((S, N, R), float("nan"), dtype=T)
    for a in used:
        a_pool[a] = torch.from_numpy(ai[a] * a_unit).to(T)
        b_pool[a] = torch.from_numpy(bi[a] * b_unit).to(T)
        assert np.array_equal(f64(a_pool[a]), ai[a] * a_unit) and np.array_equal(f64(b_pool[a]), bi[a] * b_unit)
    assert np.array_equal(f64(x_store[served, :K]), xi[served] * x_unit)
    # hT per served row in lattice units of h: x_unit * a_unit * 2^sc_e (scale_m folded into the integer)
    args = dict(ldx=ldx, total_q=total_q, a_pool=np.nan_to_num(f64(a_pool)), b_pool=np.nan_to_num(f64(b_pool)), scaling=scaling, ids=ids, cu=cu,
                max_sq=max_sq, slice_end=slice_end, dtype_name=dtype_name)
    xs64 = f64(x_store).reshape(-1)
    yi = np.zeros((total_q, N))
    yi[served] = rng.integers(-100, 101, size=(len(served), N))
    d_unit = np.ones(total_q)
    for t in served:
        d_unit[t] = x_unit * a_unit * 2.0 ** sc_e[slot[t]] * b_unit
    # d itself, exactly: steps 1 - 3 (hT rounded as the contract says)
    d = np.zeros((total_q, N))
    ends = [0] + list(slice_end)
    for a in used:
        rows = np.nonzero(slot == a)[0]
        h = (xs64.reshape(total_q, ldx)[rows, :K]) @ args["a_pool"][a].T
        hs = (np.float32(scaling[a]) * h.astype(np.float32)).astype(np.float64)
        hT = round_T(hs, dtype_name)
        hu = x_unit * a_unit * 2.0 ** sc_e[a]
        assert np.array_equal(hT / hu, np.rint(hT / hu)), "hT left the lattice"
        for j in range(ns):
            lo, hi = ends[j], ends[j + 1]
            Bj = args["b_pool"][a][lo:hi]
            assert ((np.abs(hT[:, j * R:(j + 1) * R]) / hu) @ (np.abs(Bj) / b_unit).T).max() < 2 ** 24, "not a lattice case: a partial sum of d could round"
            d[np.ix_(rows, np.arange(lo, hi))] = hT[:, j * R:(j + 1) * R] @ Bj.T
    di = d / d_unit[:, None]
    assert np.array_equal(di, np.rint(di))
    # two final y values on ties: the first served elements where some T-exact integer y puts y + d half way, one up, one down
    cand = _t_integers(dtype_name)
    cand = cand[np.argsort(np.abs(cand), kind="stable")]      # the smallest |y| that does it
    y_ties = {}
    for t in served:
        for n in range(N):
            if len(y_ties) == 2:
                break
            for want in ("up", "down"):
                if want in y_ties or (t, n) in y_ties.values():
                    continue
                for yv in cand:
                    if tie_direction(int(yv + di[t, n]), dtype_name) == want:
                        yi[t, n] = yv
                        y_ties[want] = (int(t), n)
                        break
    assert len(y_ties) == 2, "the y ties could not be placed"
    assert (np.abs(yi) + np.abs(di)).max() < 2 ** 24, "not a lattice case: y + d could round before the rounding to T"
    y_vals = yi * d_unit[:, None]
    sent = (0x3C00 + (np.arange(total_q)[:, None] * 131 + np.arange(N)[None, :] * 7) % 997).astype(np.int16)
    y_init = torch.from_numpy(sent).view(T).clone()
    y_init[served] = torch.from_numpy(y_vals[served]).to(T)
    assert np.array_equal(f64(y_init[served]), y_vals[served]), "y is not made of T values"
    case = dict(K=K, R=R, N=N, slice_end=tuple(slice_end), S=S, B=B, total_q=total_q, max_sq=max_sq, ldx=ldx, dtype_name=dtype_name, x_store=x_store,
                a_pool=a_pool, b_pool=b_pool, scaling=torch.from_numpy(scaling), ids=ids, cu=cu, y_init=y_init, served=served, slot=slot,
                h_ties=(t0, tuple(h_ties)), y_ties=y_ties, lattice=True, scale_m=scale_m, h_unit=x_unit * a_unit, d_unit=d_unit)
    case["expected"] = expected_bits(case)
    return case


def oracle_args(case):
    """the float64 view of a case that `reference` takes (NaN kept where the case holds NaN)"""
    return dict(x_store=f64(case["x_store"]).reshape(-1), ldx=case["ldx"], total_q=case["total_q"], a_pool=f64(case["a_pool"]),
                b_pool=f64(case["b_pool"]), scaling=case["scaling"].numpy(), ids=case["ids"], cu=case["cu"], max_sq=case["max_sq"],
                slice_end=case["slice_end"], y_init=f64(case["y_init"]), dtype_name=case["dtype_name"])


def expected_bits(case, mutant=None, kplan=None):
    """the T tensor a lattice case must produce: y_init with the rows the (mutant) contract serves replaced by its values"""
    args = oracle_args(case)
    y, _ = reference(mutant=mutant, kplan=kplan, **args)
    slot = row_slots(case["ids"], case["cu"], case["B"], case["total_q"], case["max_sq"], case["S"], mutant)
    out = case["y_init"].clone()
    rows = np.nonzero(slot >= 0)[0]
    out[rows] = torch.from_numpy(y[rows]).to(out.dtype)
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def build_random(K, R, N, slice_end, dtype_name, sq=None, ids=None, pad=0, rect=None, S=3, seed=0):
    """A case of ordinary random T values (x ~ N(0, 1), A ~ N(0, 1 / K), B ~ N(0, 0.05^2), y ~ N(0, 1), scaling = alpha / r of common adapters) with
    the ideal result and the derived bound.  Untouched rows as in build_lattice."""
    rng = np.random.default_rng(seed + K + 3 * N + 5 * R)
    T = DTYPES[dtype_name]
    ns = len(slice_end)
    if rect is not None:
        B, rows = rect
        cu, total_q, max_sq = None, B * rows, rows
        ids = np.array([b % S for b in range(B)] if ids is None else ids, dtype=np.int32)
    else:
        cu, total_q = layout(sq, pad)
        B, ids, max_sq = len(sq), np.array(ids, dtype=np.int32), max(sq)
    slot = row_slots(ids, cu, B, total_q, max_sq, S)
    served = np.nonzero(slot >= 0)[0]
    ldx = K + 8
    x_store = torch.full((total_q, ldx), float("nan"), dtype=T)
    x_store[served, :K] = torch.from_numpy(rng.standard_normal((len(served), K))).to(T)
    a_pool = torch.from_numpy(rng.standard_normal((S, R * ns, K)) / np.sqrt(K)).to(T)
    b_pool = torch.from_numpy(0.05 * rng.standard_normal((S, N, R))).to(T)
    scaling = torch.tensor([2.0, 0.5, 32.0 / 12.0, 1.0, 16.0 / 24.0][:S], dtype=torch.float32)
    sent = (0x3C00 + (np.arange(total_q)[:, None] * 131 + np.arange(N)[None, :] * 7) % 997).astype(np.int16)
    y_init = torch.from_numpy(sent).view(T).clone()
    y_init[served] = torch.from_numpy(rng.standard_normal((len(served), N))).to(T)
    case = dict(K=K, R=R, N=N, slice_end=tuple(slice_end), S=S, B=B, total_q=total_q, max_sq=max_sq, ldx=ldx, dtype_name=dtype_name, x_store=x_store,
                a_pool=a_pool, b_pool=b_pool, scaling=scaling, ids=ids, cu=cu, y_init=y_init, served=served, slot=slot, lattice=False)
    case["ideal"], case["bound"] = reference(ideal=True, **oracle_args(case))
    return case


def check_random(case, y):
    """y (a T tensor [total_q, N]) against a random case: untouched rows bit for bit, served rows within the bound.  Returns the largest ratio
    |y - y*| / bound over the served elements."""
    served = case["served"]
    rest = np.setdiff1d(np.arange(case["total_q"]), served)
    assert torch.equal(bits(y)[rest], bits(case["y_init"])[rest]), "a row outside the contract changed"
    err = np.abs(f64(y)[served] - case["ideal"][served])
    ratio = float((err / case["bound"][served]).max())
    assert np.isfinite(f64(y)[served]).all() and ratio <= 1.0, f"beyond the derived bound: {ratio:.3f} x"
    return ratio
