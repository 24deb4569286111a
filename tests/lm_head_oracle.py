"""numpy restatement of the LM-head contract (include/awq_cdna4.h: awq_lm_head, awq_embed_tokens; DESIGN.md "LM head") in float64, the builders of
the test cases, and the per-element bound.

The contract, per row b of x (T = bf16 or fp16):
  0. seqlens[b] < 0: out[b, :] keeps what it held; the row's x, NaN included, changes no other row.
  1. xn[b, k] = T((f32(x[b, k]) * rstd_b) * f32(gamma[k])), rstd_b = rsqrtf(sum_k x^2 / (float)K + eps), the sum in fp32; without gamma xn = x.
     `reference` is handed xn as T values (`norm` below restates the step; on the GPU the fused launch is compared bit for bit with
     ops.rmsnorm + the plain launch instead, because rsqrtf is not a correctly rounded function one can restate).
  2. y[b, v] = sum_k f32(xn[b, k]) * f32(W[v, k]) in fp32, then + f32(bias[v]) in fp32.
  3. fp32 output stores y; T output stores y rounded once to T, nearest-even.

The bound (derived, not measured).  A product of two T values has at most 22 significant bits: it is exact in fp32.  A sum of K exact terms taken in
ANY order with one rounding per addition (unit roundoff u = 2^-24) has an error of at most gamma_(K-1) * sum_k |xn w| <= K u sum_k |xn w| (Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2; the (1 + u)^K - 1 <= K u / (1 - K u) slack is below 1e-3 of the bound for K <= 16384
and is absorbed by using K where K - 1 would do), and the bias add is one more rounding of a value bounded by sum |xn w| + |bias|, hence
      |y - y64| <= (K + 1) * 2^-24 * (sum_k |xn w| + |bias|).
For T output the stored value is within half an ulp of T of y: ulp_T(|y64| + bound) / 2 is added.  The matrix unit (v_mfma_f32_16x16x32) adds 32
products to an fp32 accumulator per instruction; any grouping of the adds is covered by "any order", and adding several products with fewer
roundings than one per term only lowers the error, so the constant is kept as it stands.

On the integer lattice (x, W, bias = small integers times a power of two with sum |x||w| + |bias| < 2^24 lattice units) every partial sum is an
integer below 2^24 lattice units: exact in fp32 in any order.  The bound there is ZERO: fp32 output equals y64, T output its nearest-even rounding.
"""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PREC = {"bf16": 8, "fp16": 11}        # significant bits of T
EMIN = {"bf16": -126, "fp16": -14}    # exponent of the smallest normal number
K_STEP = 64                           # the kernel's k step (the "k tail" mutant drops K % K_STEP columns)
M_TILE = 16                           # rows of x per matrix instruction (the "NaN leak" mutant poisons the rows that share one)
R = 120                               # lattice integers are in [-R, R]: 1032 * R * R + bias < 2^24
X_EXP, W_EXP = -3, -6                 # x = integers * 2^-3, W = integers * 2^-6, y and bias in units of 2^-9

# (M, V, K): every K in {8, 40, 72, 136, 1032}, V in {1, 15, 16, 17, 127, 1025} and M in {1, 2, 7, 15, 16, 17, 33, 64} at least twice
LATTICE_SHAPES = [(1, 1, 8), (2, 15, 40), (7, 16, 72), (15, 17, 136), (16, 127, 1032), (17, 1025, 8), (33, 1, 40), (64, 15, 72), (1, 16, 136),
                  (2, 17, 1032), (7, 127, 8), (15, 1025, 40), (16, 1, 72), (17, 15, 136), (33, 16, 1032), (64, 17, 8), (64, 1025, 1032),
                  (1, 127, 40), (33, 1025, 136), (64, 127, 72), (1, 1025, 1032), (16, 17, 40)]
RANDOM_SHAPES = [(1, 1025, 4096), (8, 2000, 4096), (64, 513, 8192)]
NORM_SHAPES = [(5, 130, 72), (17, 65, 1032), (64, 33, 136)]
EPS = (0.0, 1e-6, 1e-2)
MUTANTS = ("k_tail", "v_tail", "row_prev", "ldx_as_k", "no_gamma", "eps_outside", "xn_unrounded", "bias_per_split", "bias_T_first", "trunc",
           "inactive_written", "nan_leak")


def f64(t):
    """a torch tensor of T (or fp32) values as float64, exactly"""
    return t.detach().cpu().float().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def ulp_T(a, dtype_name):
    """spacing of T at magnitude |a| (float64 array)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** EMIN[dtype_name])))
    return 2.0 ** (e - (PREC[dtype_name] - 1))


def round_T(y, dtype_name, truncate=False):
    """float64 -> the nearest T value, ties to even (truncate: toward zero), as float64.  Finite values inside T's range."""
    y = np.asarray(y, dtype=np.float64)
    u = ulp_T(y, dtype_name)
    q = y / u                                   # exact: u is a power of two
    r = np.trunc(q) if truncate else np.rint(q)  # np.rint rounds halves to even
    return r * u


def norm(x, gamma, eps, dtype_name, mutant=None):
    """step 1 in numpy: x, gamma float64 arrays of T values -> xn as T values (float64).  fp32 arithmetic, the sum of squares exact on lattice rows."""
    K = x.shape[-1]
    ss = (x * x).sum(-1).astype(np.float32)
    if mutant == "eps_outside":
        rstd = (np.float32(1.0) / np.sqrt(ss / np.float32(K))).astype(np.float32) + np.float32(eps)
    else:
        rstd = (np.float32(1.0) / np.sqrt(ss / np.float32(K) + np.float32(eps))).astype(np.float32)
    g = np.ones_like(gamma) if mutant == "no_gamma" else gamma
    xn = (x.astype(np.float32) * rstd[..., None]).astype(np.float32) * g.astype(np.float32)
    return xn.astype(np.float64) if mutant == "xn_unrounded" else round_T(xn.astype(np.float64), dtype_name)


def rows_of(x_store, M, K, ldx):
    """the M rows of x out of its storage: row b starts at element b * ldx"""
    flat = np.asarray(x_store).reshape(-1)
    return np.stack([flat[b * ldx: b * ldx + K] for b in range(M)])


def reference(x_store, ldx, M, w, bias=None, gamma=None, eps=0.0, seqlens=None, out_init=None, out="f32", dtype_name="bf16", mutant=None, splits=4,
              tile=64):
    """steps 0 - 3 in float64.  x_store: float64 array holding the storage of x's M rows (row b at b * ldx), w [V, K], bias [V], gamma [K] as float64 arrays of T
    values; out: "f32" or "T"; out_init [M, V] is what the output held before.  Returns (y [M, V], absdot [M, V] = sum |xn w| + |bias|)."""
    V, K = w.shape
    x = rows_of(x_store, M, K, K if mutant == "ldx_as_k" else ldx)
    if mutant == "row_prev":
        x = np.concatenate([x[:1], x[:-1]])
    xn = norm(x, gamma, eps, dtype_name, mutant) if gamma is not None else x
    active = np.ones(M, bool) if seqlens is None else np.asarray(seqlens) >= 0
    if mutant == "nan_leak":
        xn = xn.copy()
        for b in np.nonzero(~active)[0]:
            if np.isnan(xn[b]).any():
                xn[b // M_TILE * M_TILE: b // M_TILE * M_TILE + M_TILE] = np.nan
    kk = K - K % K_STEP if mutant == "k_tail" else K
    with np.errstate(invalid="ignore"):
        y = xn[:, :kk] @ w[:, :kk].T
        absdot = np.abs(xn) @ np.abs(w).T
    if bias is not None:
        if mutant == "bias_per_split":
            y = y + splits * bias
        elif mutant == "bias_T_first":
            y = round_T(y, dtype_name) + bias
        else:
            y = y + bias
        absdot = absdot + np.abs(bias)
    if out == "T":
        with np.errstate(invalid="ignore"):
            y = np.where(np.isfinite(y), round_T(np.nan_to_num(y), dtype_name, truncate=mutant == "trunc"), y)
    res = np.zeros((M, V)) if out_init is None else np.array(out_init, dtype=np.float64)
    keep = active | (mutant == "inactive_written")
    vend = V - V % tile if mutant == "v_tail" else V
    res[np.ix_(keep, np.arange(V) < vend)] = y[np.ix_(keep, np.arange(V) < vend)]
    return res, absdot


def bound(absdot, K, out="f32", dtype_name="bf16", y=None):
    """the docstring's per-element bound for general inputs"""
    b = (K + 1) * 2.0 ** -24 * absdot
    return b + (ulp_T(np.abs(y) + b, dtype_name) / 2 if out == "T" else 0.0)


def embed_reference(tokens, table):
    tokens = np.asarray(tokens).astype(np.int64)
    out = np.zeros((tokens.size, table.shape[1]), dtype=table.dtype)
    ok = (tokens >= 0) & (tokens < table.shape[0])
    out[ok] = table[tokens[ok]]
    return out


# ---- builders ----

def _tie_target(s, dtype_name, up):
    """the tie point of T nearest below |s| whose nearest-even rounding goes up (odd n) or down (even n); None where T still holds every integer"""
    p = PREC[dtype_name]
    a = abs(s)
    if a < 2 ** (p + 1):
        return None
    e = int(np.floor(np.log2(a)))
    ulp = 2 ** (e - (p - 1))
    n = int(a // ulp)
    if (n % 2 == 1) != up:
        n -= 1
    if n * ulp < 2 ** e:          # left the binade: the spacing would change
        n += 2
    return int(np.sign(s)) * (n * ulp + ulp // 2)


def build_lattice(M, V, K, dtype_name, with_bias, seed=0):
    """x [M, 3, K] whose last token holds lattice values and whose other tokens are NaN (ldx = 3 K), W [V, K], bias [V]: integers in [-R, R] times a
    power of two, so that y is exact in fp32 in any order; columns 0 and 1 of row 0 are moved onto ties of T (one rounds up, one down) where the
    sums are large enough to have any.  Returns a dict of torch tensors (CPU) and the float64 expectations."""
    rng = np.random.default_rng(1000 * seed + 7 * M + 13 * V + K + (1 if with_bias else 0) + (500 if dtype_name == "fp16" else 0))
    xi = rng.integers(-R, R + 1, size=(M, K)).astype(np.float64)
    wi = rng.integers(-R, R + 1, size=(V, K)).astype(np.float64)
    bi = rng.integers(-R, R + 1, size=V).astype(np.float64) if with_bias else None
    xi[0, 0], xi[0, 1] = 64.0, 1.0
    ties = []
    for v in range(min(V, 2)):
        s = float(xi[0] @ wi[v] + (bi[v] if with_bias else 0.0))
        t = _tie_target(s, dtype_name, up=(v == 0))
        if t is None:
            continue
        d = t - s
        a = int(np.rint(d / 64.0))
        b = int(d - 64 * a)
        if abs(wi[v, 0] + a) <= 255 and abs(wi[v, 1] + b) <= 255:   # eight significant bits: a T value in both formats
            wi[v, 0] += a
            wi[v, 1] += b
            ties.append(v)
    absdot = np.abs(xi) @ np.abs(wi).T + (np.abs(bi) if with_bias else 0.0)
    assert absdot.max() < 2 ** 24, "not a lattice case: a partial sum could round"
    T = DTYPES[dtype_name]
    x3 = torch.full((M, 3, K), float("nan"), dtype=T)
    x3[:, 2, :] = torch.from_numpy(xi * 2.0 ** X_EXP).to(T)
    w = torch.from_numpy(wi * 2.0 ** W_EXP).to(T)
    bias = torch.from_numpy(bi * 2.0 ** (X_EXP + W_EXP)).to(T) if with_bias else None
    assert np.array_equal(f64(x3[:, 2, :]), xi * 2.0 ** X_EXP) and np.array_equal(f64(w), wi * 2.0 ** W_EXP)
    assert bias is None or np.array_equal(f64(bias), bi * 2.0 ** (X_EXP + W_EXP))
    case = dict(M=M, V=V, K=K, dtype_name=dtype_name, x3=x3, w=w, bias=bias, ldx=3 * K, ties=ties)   # ties: the columns of row 0 that sit on a tie
    store = f64(x3).reshape(-1)[2 * K:]            # storage seen from the last token of row 0 on
    case["x_store"] = store
    for out in ("f32", "T"):
        case["y_" + out] = reference(store, 3 * K, M, f64(w), None if bias is None else f64(bias), out=out, dtype_name=dtype_name,
                                     out_init=np.zeros((M, V)))[0]
    return case


def build_norm_lattice(M, V, K, dtype_name, eps, seed=0):
    """rows for fused norm = unfused norm: x integers in [-R, R] (K R^2 < 2^24: the sum of squares is exact in fp32 in any order); row 0 is tiny,
    with a variance of the order of eps, so that eps decides its rstd.  W and gamma are ordinary random T values."""
    rng = np.random.default_rng(seed + M + 3 * V + 5 * K)
    xi = rng.integers(-R, R + 1, size=(M, K)).astype(np.float64)
    assert K * R * R < 2 ** 24
    T = DTYPES[dtype_name]
    scale = np.ones((M, 1))
    if eps > 0:
        scale[0, 0] = 2.0 ** np.round(np.log2(np.sqrt(eps) / (R * 0.58)))   # rms of a uniform integer row is ~0.58 R
    x = torch.from_numpy(xi * scale).to(T)
    assert np.array_equal(f64(x), xi * scale)
    gamma = torch.from_numpy(1.0 + 0.1 * rng.standard_normal(K)).to(T)
    w = torch.from_numpy(0.02 * rng.standard_normal((V, K))).to(T)
    return dict(M=M, V=V, K=K, dtype_name=dtype_name, eps=eps, x=x, gamma=gamma, w=w)


def inactive_patterns(M):
    """seqlens with -1 at the first, a middle and the last row"""
    out = []
    for b in (0, M // 2, M - 1):
        s = np.arange(1, M + 1, dtype=np.int32)
        s[b] = -1
        out.append(s)
    return out


def planned_v(plan, k=64, m=2):
    """a V whose tiles outnumber the plan's own grid (so some block walks at least two tiles) and whose last tile is partial"""
    t = plan(m, 1, k)["tile_rows"]
    for n in range(2, 1 << 14):
        v = (n - 1) * t + 17
        if plan(m, v, k)["blocks"] < n:
            return v
    raise AssertionError("no V found")
