"""float64 / integer restatements of the elementwise tails every token passes through (no GPU, none of this project's kernels):

  * SiLU * mul (fused_mlp.py:79-82): c = T(T(silu(gate)) * up), silu evaluated in fp32 on the T-valued gate  -> silu_hull, tail_accept
  * fp32 -> T rounding (+ bias in T) of a tensor-parallel row split: T(T(y) + b)                             -> rne_to_T, round_bias_ref
  * the inputs that pin them: every bit pattern of T as a gate, every rounding tie of fp32 -> T              -> all_patterns, rounding_patterns
  * selector weights that put a chosen (gate, up) pair in front of a fused GEMM epilogue                     -> selector_case

Everything is computed from bit patterns and float64, so the same tables come out on every host."""
import numpy as np
import torch

from oracle import awq_oracle as O

MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}
T_MAX = {torch.float16: 65504.0, torch.bfloat16: float(2.0 ** 127 * (2.0 - 2.0 ** -7))}
SILU_MIN_AT = -1.2784645427610738  # argmin of x / (1 + e^-x)


# ---------------- bit patterns ----------------
def from_bits(bits, dtype) -> torch.Tensor:
    """uint16 patterns (any integer array-like) -> T tensor"""
    b = np.asarray(bits).astype(np.uint16)
    return torch.from_numpy(b.view(np.int16).copy()).view(dtype)


def to_bits(t: torch.Tensor) -> np.ndarray:
    """T tensor -> uint16 patterns"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def all_patterns(dtype) -> torch.Tensor:
    """the 65536 values of T in pattern order"""
    return from_bits(np.arange(65536), dtype)


def f32_from_bits(bits) -> torch.Tensor:
    return torch.from_numpy(np.asarray(bits).astype(np.uint32).view(np.float32).copy())


def one_ulp(dtype) -> float:
    return 2.0 ** -MANT[dtype]


def smallest_normal(dtype) -> float:
    return 2.0 ** MIN_EXP[dtype]


def smallest_subnormal(dtype) -> float:
    return 2.0 ** (MIN_EXP[dtype] - MANT[dtype])


# ---------------- float64 -> T, one RNE rounding (torch's double -> bf16 goes through fp32: two roundings) ----------------
def rne64_to_T(v, dtype) -> torch.Tensor:
    """one round-to-nearest-even of float64 values to T: subnormals, overflow to inf (from T_max + half an ulp on), the sign of zero kept,
    NaN -> NaN.  The rounded value is formed exactly in float64 (an integer number of quanta of the binade), so the final cast is exact."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    fin = np.isfinite(v)
    af = np.where(fin, a, 1.0)
    _m, ex = np.frexp(af)                                   # af = m 2^ex, m in [0.5, 1): the binade starts at 2^(ex - 1)
    p = np.maximum(ex - 1, MIN_EXP[dtype]).astype(np.float64)
    quantum = np.exp2(p - MANT[dtype])
    r = np.rint(af / quantum) * quantum                      # (np.rint rounds halves to even; the division by a power of two is exact)
    r = np.where(r > T_MAX[dtype], np.inf, r)
    r = np.where(fin, r, a)                                  # inf stays inf, NaN stays NaN
    r = np.copysign(r, v)
    out = torch.from_numpy(r).to(dtype)
    assert bool(np.array_equal(out.double().numpy(), r, equal_nan=True)), "the rounded value must be exact in T"
    return out


# ---------------- SiLU ----------------
def silu64(x: np.ndarray) -> np.ndarray:
    """x / (1 + exp(-x)) in float64: +-0 -> +-0, NaN -> NaN, +inf -> +inf, -inf -> NaN (-inf / inf: NOT pinned, see silu_hull)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return x / (1.0 + np.exp(-x))


def silu_delta(x: np.ndarray) -> np.ndarray:
    """(4 + |x| w(x)) 2^-23 with w = e^-x / (1 + e^-x) <= 1: see silu_hull"""
    with np.errstate(over="ignore", invalid="ignore"):
        w = 1.0 / (1.0 + np.exp(x))
    w = np.where(np.isinf(x), np.where(x > 0, 0.0, 1.0), w)
    with np.errstate(invalid="ignore"):
        return (4.0 + np.where(w == 0, 0.0, np.abs(x) * w)) * 2.0 ** -23


def silu_hull(gate: torch.Tensor):
    """(lo, hi) T tensors: the values T(silu(gate)) may take when silu is evaluated in fp32 as x * rcp(1 + exp2(-x log2 e)) on the hardware
    transcendentals.  e = x / (1 + exp(-x)) in float64, lo = RNE_T(e (1 - delta)), hi = RNE_T(e (1 + delta)), ordered by value, with

        delta(x) = (4 + |x| w) 2^-23,   w = e^-x / (1 + e^-x)   (<= (4 + |x|) 2^-23).

    Derivation (relative errors; one fp32 ulp = 2^-23, half an ulp = 2^-24):
      * the product x log2 e is rounded once: an absolute error of |x log2 e| 2^-24 in the exponent, which is |x| 2^-24 relative in the
        exponential; the constant log2 e is itself rounded to fp32 (2^-25.6 relative) -- together below |x| 2^-23 in e^-x;
      * an error of the exponential reaches 1 / (1 + e^-x) multiplied by w = e^-x / (1 + e^-x): this is the factor on |x|.  Without it the bound
        would be (4 + |x|) 2^-23, which no longer pins a code from |x| = 2^(23 - MANT) on (delta alone exceeds an ulp of T) although the code
        returns x exactly there (1 + e^-x rounds to 1); with it lo and hi are never more than one code apart over all of T;
      * v_exp_f32 and v_rcp_f32 are taken at 1 ulp each: 2 x 2^-23;
      * the add 1 + e^-x and the two multiplies round to nearest, half an ulp each: 3 x 2^-24 < 2 x 2^-23;
      * the 2^-64 scalings below x = -64 are exact powers of two.  (The last one can land on an fp32 subnormal -- silu below 2^-126, gates under
        -87.3 in bf16 -- where fp32 rounds to a multiple of 2^-149, 2^16 times finer than bf16's subnormal spacing.)
    +-0 -> +-0, NaN -> NaN, +inf -> +inf.  -inf is not pinned (the code computes -inf * 0): lo = hi = NaN there and the callers mask it."""
    x = gate.double().numpy()
    e = silu64(x)
    d = silu_delta(x)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = e * (1.0 - d), e * (1.0 + d)
    a = np.where((e == 0) | np.isinf(e), e, a)  # (keeps the sign of zero and +inf)
    b = np.where((e == 0) | np.isinf(e), e, b)
    lo64, hi64 = np.fmin(a, b), np.fmax(a, b)
    lo64 = np.where(np.isnan(e), np.nan, lo64)
    hi64 = np.where(np.isnan(e), np.nan, hi64)
    return rne64_to_T(lo64, gate.dtype), rne64_to_T(hi64, gate.dtype)


def tail_accept(gate: torch.Tensor, up: torch.Tensor):
    """(c_lo, c_hi) T tensors: the two acceptable results of T(T(silu(gate)) * up), one per end of silu_hull.  The product of two T values is exact
    in float64 and is rounded once to T.  (inf * 0 and anything with NaN give NaN; -inf gates give NaN here and are masked by the callers.)"""
    lo, hi = silu_hull(gate)
    u = up.double().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        return rne64_to_T(lo.double().numpy() * u, gate.dtype), rne64_to_T(hi.double().numpy() * u, gate.dtype)


def bits_equal_or_nan(out: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """bool mask (on out's device): same bit pattern (so the sign of zero and of inf count), or both NaN"""
    want = want.to(out.device)
    return (out.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(out) & torch.isnan(want))


def tail_check(out: torch.Tensor, c_lo: torch.Tensor, c_hi: torch.Tensor):
    """-> (bad mask, took_lo, took_hi): an output is accepted when its bits are those of c_lo or of c_hi (NaN: when the reference is NaN);
    took_lo / took_hi count the outputs on one end only, where the two ends differ"""
    a, b = bits_equal_or_nan(out, c_lo), bits_equal_or_nan(out, c_hi)
    amb = ~bits_equal_or_nan(c_lo.to(out.device), c_hi)
    return ~(a | b), int((a & amb).sum().item()), int((b & amb).sum().item())


# ---------------- fp32 -> T, integer arithmetic ----------------
def rne_to_T(f32: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 -> T round-to-nearest-even on the bit patterns (numpy integers): subnormal results, overflow to inf, NaN stays NaN (quiet)"""
    u = f32.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    sign = (u >> 31) & 1
    a = u & 0x7FFFFFFF
    nan = a > 0x7F800000
    if dtype == torch.bfloat16:
        h = (a + 0x7FFF + ((a >> 16) & 1)) >> 16   # the exponent fields coincide: a carry out of the mantissa is the next binade, or inf
        h = np.where(nan, 0x7FC0, h)
    else:
        exp = a >> 23
        man = a & 0x7FFFFF
        # normal results (|v| >= 2^-14): rebias, keep 10 bits, round on the 13 dropped ones; a carry runs into the exponent, 0x7C00 = inf
        hn = ((np.maximum(exp, 113) - 112) << 10) | (man >> 13)
        rem = man & 0x1FFF
        hn = hn + ((rem > 0x1000) | ((rem == 0x1000) & ((hn & 1) == 1)))
        hn = np.minimum(hn, 0x7C00)
        # subnormal results: the 24-bit significand in units of 2^(exp - 150), wanted in units of 2^-24
        sig = np.where(exp == 0, man, man | 0x800000)
        sh = np.minimum(126 - np.minimum(np.maximum(exp, 1), 125), 40).astype(np.uint64)
        hs = sig >> sh
        rems = sig & ((np.uint64(1) << sh) - np.uint64(1))
        half = np.uint64(1) << (sh - np.uint64(1))
        hs = hs + ((rems > half) | ((rems == half) & ((hs & 1) == 1)))
        h = np.where(exp >= 113, hn, hs)
        h = np.where(nan, 0x7E00, h)
    return from_bits((h | (sign << 15)).astype(np.uint16), dtype)


def round_bias_ref(y32: torch.Tensor, bias, dtype) -> torch.Tensor:
    """T(T(y) + b): rne_to_T, an fp32 add of the two T values (exact or one fp32 rounding), rne_to_T again -- what `y.to(T) + b` means.
    (T + T rounded to fp32 and then to T equals the single rounding of the exact sum: fp32 carries more than 2 * MANT + 2 bits.)"""
    y = rne_to_T(y32, dtype)
    if bias is None:
        return y
    n = bias.numel()
    s = (y.float().reshape(-1, n) + bias.float().reshape(1, n)).reshape(y32.shape)
    return rne_to_T(s, dtype)


def rounding_patterns(dtype) -> torch.Tensor:
    """fp32 inputs at which a conversion to T can go wrong: for every finite t >= 0 of T and its successor t' (inf's place after T_max) the
    midpoint and the midpoint -+ one fp32 ulp, in both signs (these hold the overflow threshold T_max + half an ulp and the tie at half the
    smallest subnormal, listed again explicitly with their neighbours); for bf16 a spread of fp32 denormals; +-0, +-inf, quiet and signalling
    NaN patterns.  Padded with 1.0 to a multiple of 8."""
    if dtype == torch.bfloat16:
        mid = (np.arange(0x7F80, dtype=np.uint64) << 16) + 0x8000
        thr = 0x7F7F8000
        tie = 0x00008000   # 2^-134: half of bf16's smallest subnormal 2^-133 (an fp32 denormal)
    else:
        t = from_bits(np.arange(0x7C00), dtype).double().numpy()
        nxt = np.append(t[1:], 65536.0)
        mid = torch.from_numpy(((t + nxt) / 2).astype(np.float32)).view(torch.int32).numpy().astype(np.uint64)
        assert np.array_equal(f32_from_bits(mid).double().numpy(), (t + nxt) / 2), "fp16 midpoints are exact in fp32"
        thr = 0x477FF000   # 65520
        tie = 0x33000000   # 2^-25
    pos = [mid - 1, mid, mid + 1, np.array([thr - 1, thr, thr + 1, tie - 1, tie, tie + 1], dtype=np.uint64)]
    if dtype == torch.bfloat16:
        den = np.array([1, 2, 3, 0x7FFF, 0x8001, 0xFFFF, 0x10000, 0x17FFF, 0x18000, 0x18001, 0x3FFFFF, 0x400000, 0x7F7FFF, 0x7F8000, 0x7FFFFF],
                       dtype=np.uint64)
        rng = np.random.Generator(np.random.PCG64(20240607))
        pos += [den, rng.integers(1, 0x800000, size=241).astype(np.uint64)]
    pos = np.concatenate(pos)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0x7FFFFFFF, 0xFFFFFFFF],
                       dtype=np.uint64)
    allb = np.concatenate([pos, pos | 0x80000000, special])
    pad = (-len(allb)) % 8
    allb = np.concatenate([allb, np.full(pad, 0x3F800000, dtype=np.uint64)])
    return f32_from_bits(allb)


# ---------------- selector weights: any (gate, up) pair in front of any fused epilogue ----------------
def selector_case(K, F, dtype, bits=4):
    """-> dict(gate=case, up=case), each in make_lattice_case's form (N = F, K, bits, q uint8 [F, K], z [G, F], s [G, F], scales /
    scaled_zeros T [Gpad, F]): weights (q - z) s with s = 1, z = 8 (W3: 4) and q = z everywhere except ONE k per column where q = z + 1 --
    gate column n at k = 2 (n mod K/2), up column n at k = 2 (n mod K/2) + 1.  Then, with j = n mod K/2,

        gate'[m, n] = x[m, 2 j]      up'[m, n] = x[m, 2 j + 1]

    exactly in fp32 in any summation order for finite x: every other term is x * 0 = +-0 (x = -0 comes out as +0 once a +0 is in the sum:
    selector_pairs).  The scales are asserted exact in T."""
    assert K % 128 == 0 and F % 16 == 0
    G = K // 128
    zc = 8 if bits == 4 else 4
    n = np.arange(F)
    out = {}
    for name, odd in (("gate", 0), ("up", 1)):
        q = np.full((F, K), zc, dtype=np.uint8)
        q[n, 2 * (n % (K // 2)) + odd] = zc + 1
        z = np.full((G, F), zc, dtype=np.uint8)
        s = np.ones((G, F), dtype=np.float64)
        gp = O.padded_groups(K)
        sc = torch.zeros(gp, F, dtype=torch.float64)
        sc[:G] = 1.0
        szd = torch.zeros(gp, F, dtype=torch.float64)
        szd[:G] = -float(zc)
        scales, scaled_zeros = sc.to(dtype), szd.to(dtype)
        assert torch.equal(scales.double(), sc) and torch.equal(scaled_zeros.double(), szd), "selector scales must be exact in T"
        out[name] = dict(N=F, K=K, dtype=dtype, bits=bits, q=q, z=z, s=s, scales=scales, scaled_zeros=scaled_zeros)
    return out


def selector_x(gates: torch.Tensor, ups: torch.Tensor, K: int) -> torch.Tensor:
    """x [rows, K] holding the pairs (gates[i], ups[i]) at columns (2 j, 2 j + 1); the last row is filled up by repeating the first pairs"""
    per = K // 2
    n = gates.numel()
    rows = -(-n // per)
    idx = torch.arange(rows * per) % n
    x = torch.stack([gates.reshape(-1)[idx], ups.reshape(-1)[idx]], -1)
    return x.reshape(rows, K).contiguous()


def selector_pairs(x: torch.Tensor, F: int, swapped: bool = False):
    """the (gate', up') [rows, F] a correct kernel forms from x under selector_case's weights: x[m, 2 j] and x[m, 2 j + 1], j = n mod K/2, plus
    the +0 of the other terms (-0 + +0 = +0 in round-to-nearest: a -0 input arrives as +0).  `swapped`: the de-interleave mutant."""
    K = x.shape[-1]
    j = torch.arange(F) % (K // 2)
    g, u = x[:, 2 * j], x[:, 2 * j + 1]
    if swapped:
        g, u = u, g
    return (g.float() + 0.0).to(x.dtype), (u.float() + 0.0).to(x.dtype)


# ---------------- the inputs of tests/test_gpu_tails.py (and of the mutants of tests/test_tail_host.py: the same tables) ----------------
SILU_FIRST_TRIP = 8192 * 256 * 8        # elements the capped grid of silu_mul_kernel / silu_mul_interleaved_kernel covers in one trip
SILU_SECOND_TRIP = SILU_FIRST_TRIP + 8 * 257
ROUND_FIRST_TRIP = 4096 * 256 * 8       # round_bias_f32_kernel
ROUND_BIG = (2056, 4104)                # 8 437 824 elements: a second trip, a row length that is no power of two


def _gen(seed):
    from tests.helpers import Gen
    return Gen(seed)


def finite_patterns(dtype, count, seed) -> torch.Tensor:
    """`count` finite T values drawn uniformly over the bit patterns (every binade, subnormals included)"""
    b = _gen(seed).g.integers(0, 65536, size=4 * count).astype(np.uint16)
    t = from_bits(b, dtype)
    return t[torch.isfinite(t.float())][:count].clone()


def up_values(dtype) -> torch.Tensor:
    """the 64 `up` values of the standalone sweep: the edges of T, full mantissas, inf / NaN, and finite patterns from a fixed seed"""
    u, sn, ss, tm = one_ulp(dtype), smallest_normal(dtype), smallest_subnormal(dtype), T_MAX[dtype]
    fixed = torch.tensor([1.0, -1.0, tm, -tm, sn, -sn, ss, -ss, 0.0, -0.0, 3.0, 1.0 + u, 2.0 - u, float("inf"), float("-inf"), float("nan")],
                         dtype=torch.float64)
    fixed = rne64_to_T(fixed.numpy(), dtype)
    out = torch.cat([fixed, finite_patterns(dtype, 64 - fixed.numel(), 7001)])
    assert out.numel() == 64
    return out


def sweep_accept(dtype, ups: torch.Tensor):
    """every gate pattern x every up: (gate [65536, U], up [65536, U], c_lo, c_hi, pinned) -- pinned False on the rows of gate = -inf"""
    g = all_patterns(dtype)
    lo, hi = silu_hull(g)
    u = ups.double().numpy()[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        c_lo = rne64_to_T(lo.double().numpy()[:, None] * u, dtype)
        c_hi = rne64_to_T(hi.double().numpy()[:, None] * u, dtype)
    gate = g[:, None].expand(65536, ups.numel()).contiguous()
    up = ups[None, :].expand(65536, ups.numel()).contiguous()
    pinned = ~(torch.isinf(g.float()) & (g.float() < 0))[:, None].expand_as(gate)
    return gate, up, c_lo, c_hi, pinned


def edge_gates(dtype) -> torch.Tensor:
    """the gates driven through every fused epilogue: the band below -63 where the reciprocal needs its rescue (every value of bf16's grid down to
    -98: the nonzero bf16 results end at -97), every gate whose hull is ambiguous, every gate with a subnormal silu, every 16th pattern in
    [-20, 20], the two codes either side of the minimum at -1.2785, +-0, +- the smallest subnormal, +-T_max"""
    g = all_patterns(dtype)
    x = g.double().numpy()
    fin = np.isfinite(x)
    lo, hi = silu_hull(g)
    e_T = rne64_to_T(silu64(np.where(fin, x, 0.0)), dtype).double().numpy()
    on_bf16_grid = (to_bits(g.float().to(torch.bfloat16).to(dtype)) == to_bits(g)) if dtype != torch.bfloat16 else np.ones(65536, bool)
    pick = fin & (x >= -98) & (x <= -63) & on_bf16_grid
    pick |= fin & (to_bits(lo) != to_bits(hi))
    pick |= fin & (e_T != 0) & (np.abs(e_T) < smallest_normal(dtype))
    pick |= fin & (np.abs(x) <= 20) & (np.arange(65536) % 16 == 0)
    below = np.where(fin & (x <= SILU_MIN_AT), x, -np.inf).max()
    above = np.where(fin & (x >= SILU_MIN_AT), x, np.inf).min()
    pick |= (x == below) | (x == above)
    pick |= fin & ((x == 0) | (np.abs(x) == smallest_subnormal(dtype)) | (np.abs(x) == T_MAX[dtype]))
    return g[torch.from_numpy(pick)].clone()


def edge_pairs(dtype):
    """(gates, ups): every edge gate with up in {1, -(2 - ulp), the smallest normal}"""
    g = edge_gates(dtype)
    ups = rne64_to_T(np.array([1.0, -(2.0 - one_ulp(dtype)), smallest_normal(dtype)]), dtype)
    return g.repeat_interleave(3), ups.repeat(g.numel())


def bias_values(dtype, n, seed=7002) -> torch.Tensor:
    """a bias in T [n]: +-0, +-T_max, +- the smallest subnormal, powers of two 2^20 above and below the unit-scale inputs, the rest random patterns
    of every binade.  The fixed values sit at different positions of every octet so that a bias read one octet off is another value."""
    tm, ss = T_MAX[dtype], smallest_subnormal(dtype)
    b = finite_patterns(dtype, n, seed)
    fixed = rne64_to_T(np.array([0.0, -0.0, tm, -tm, ss, -ss, 2.0 ** 20 if dtype == torch.bfloat16 else 2.0 ** 15, 2.0 ** -20, -2.0 ** -20, 1.0, -3.0]), dtype)
    pos = (np.arange(fixed.numel()) * 9) % n if n >= 64 else np.arange(min(n, fixed.numel()))
    b[torch.from_numpy(pos)] = fixed[:len(pos)]
    return b


def round_inputs(dtype, m, n, seed=7003) -> torch.Tensor:
    """fp32 [m, n]: rounding_patterns tiled over the first rows, then random fp32 values (unit scale, and patterns of every binade of T's range)"""
    total = m * n
    pat = rounding_patterns(dtype)
    g = _gen(seed)
    y = torch.empty(total, dtype=torch.float32)
    k = min(total // 2, pat.numel())
    y[:k] = pat[:k]
    rest = total - k
    half = rest // 2
    y[k:k + half] = torch.from_numpy(g.g.standard_normal(size=half, dtype=np.float32)) * 3
    lo_e, hi_e = (0x33000000, 0x47800000) if dtype == torch.float16 else (0x00000001, 0x7F800000)
    bits = g.g.integers(lo_e, hi_e, size=rest - half).astype(np.uint32) | (g.g.integers(0, 2, size=rest - half).astype(np.uint32) << 31)
    y[k + half:] = f32_from_bits(bits)
    return y.reshape(m, n)


RMS_K = (8, 16, 2040, 2048, 2056, 4088, 16384)  # 256 threads x 8 elements: one, exactly one, and more than one trip, each with a ragged tail
RMS_EPS = 1e-6


def rmsnorm_rows(K, dtype, seed=7004):
    """(x [5, K], gamma [K]): row 0 all zero (both signs), row 1 zero but for one element equal to 1, row 2 ~ N(0, 1) 2^-12, row 3 ~ N(0, 1) 2^6,
    row 4 values near 200 -- neighbouring rows differ by orders of magnitude, so a block that used another row's partial sum misses by far more
    than the model allows.  (Rows whose fp32 sum of squares overflows are out of scope.)"""
    g = _gen(seed + K)
    x = torch.zeros(5, K, dtype=torch.float64)
    x[0] = torch.where(torch.arange(K) % 3 == 0, -0.0, 0.0).double()
    x[1, (K * 5) // 8 if K > 8 else 5] = 1.0
    x[2] = g.randn(K).double() * 2.0 ** -12
    x[3] = g.randn(K).double() * 2.0 ** 6
    x[4] = 200.0 + g.randn(K).double()
    gamma = (1 + 0.2 * g.randn(K)).double()
    gamma[1::7] *= -1
    return rne64_to_T(x.numpy(), dtype), rne64_to_T(gamma.numpy(), dtype)


def rmsnorm_ref(x: torch.Tensor, gamma: torch.Tensor, eps: float, tot=None) -> torch.Tensor:
    """T((x rstd) gamma) from float64, one rounding; `tot` [M, 1] overrides the sum of squares (the mutants)"""
    xd = x.double()
    ss = (xd * xd).sum(-1, keepdim=True) if tot is None else tot
    v = xd * torch.rsqrt(ss / x.shape[-1] + eps) * gamma.double()
    return rne64_to_T(v.numpy(), x.dtype)
