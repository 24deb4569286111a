"""The FP8 KV-cache format (DESIGN.md "FP8 KV cache"), restated in numpy alone -- nothing of llm_awq_amd is imported -- and the case lists
tests/test_gpu_kv8.py runs through the kernels.

  caches   codes [Bc, L, Hkv, Dh] uint8 (OCP e4m3fn: 1 sign, 4 exponent bits of bias 7, 3 mantissa bits, 0x7F / 0xFF = NaN, no Inf)
           scales [Bc, L, Hkv] float32
  quant    one head row x[0..Dh) of T:  s = max(max|x|, 2^-60) / 448 (fp32 division);  code = e4m3fn_RNE(clamp(x / s, -448, 448))
  dequant  T(float(code) * s): one fp32 multiply, one rounding to T

T values travel as float32 arrays that hold T-representable numbers (`round_to`) or as their uint16 bit patterns (`to_bits`).  Every
arithmetic step is a float32 numpy operation, i.e. one IEEE operation with one rounding; e4m3fn is decoded by formula and encoded by a
nearest-value search over the 127 finite non-negative values with ties to the even code, so no library's cast is trusted.

MUTANTS are wrong variants of this restatement; tests/test_kv8_host.py shows that each changes the expected results of the case lists."""
import numpy as np

F32 = np.float32
E4M3_MAX = F32(448.0)
AMAX_FLOOR = F32(2.0 ** -60)
MUTANTS = ("per_token", "k_scale_on_v", "amax_half", "trunc", "recip", "max240")


# ------------------------------------------------------------------------------------------------------------------------
# e4m3fn
# ------------------------------------------------------------------------------------------------------------------------
def _decode_one(code):
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 0xF, code & 0x7
    if e == 0xF and m == 0x7:
        return float("nan")
    if e == 0:
        return sign * m * 2.0 ** -9            # subnormal: m / 8 * 2^-6
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


DECODE = np.array([_decode_one(c) for c in range(256)], dtype=np.float32)  # exact: every value has 4 significant bits
_POS = DECODE[:127].astype(np.float64)                                      # codes 0x00 .. 0x7E, ascending, 0 .. 448


def e4m3_decode(codes):
    return DECODE[np.asarray(codes, dtype=np.uint8)]


def e4m3_encode(x, trunc=False):
    """float32 values in [-448, 448] -> codes; nearest, ties to the even code, the sign bit kept (also on a zero result).
    trunc: towards zero (a mutant)."""
    x = np.asarray(x, dtype=np.float32)
    assert not np.isnan(x).any() and (np.abs(x) <= 448).all()
    a = np.abs(x).astype(np.float64)
    hi = np.minimum(np.searchsorted(_POS, a, side="left"), 126)  # first value >= a
    lo = np.maximum(hi - 1, 0)
    if trunc:
        mag = np.where(_POS[hi] == a, hi, lo)
    else:
        twice, mid2 = 2.0 * a, _POS[lo] + _POS[hi]               # both exact in float64
        mag = np.where(twice < mid2, lo, np.where(twice > mid2, hi, np.where(lo % 2 == 0, lo, hi)))
        mag = np.where(_POS[hi] == a, hi, mag)
    return (mag | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# T = float16 / bfloat16
# ------------------------------------------------------------------------------------------------------------------------
def to_bits(x, dtype):
    """float32 -> the uint16 bit pattern of its RNE rounding to T ("f16" / "bf16"); finite inputs."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    assert dtype == "bf16"
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(b, dtype):
    b = np.asarray(b, dtype=np.uint16)
    if dtype == "f16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def round_to(x, dtype):
    return from_bits(to_bits(x, dtype), dtype)


def ulp(x, dtype):
    """The spacing of T at |x| (the subnormal spacing below the smallest normal)."""
    p, emin = (10, -14) if dtype == "f16" else (7, -126)
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - p)


# ------------------------------------------------------------------------------------------------------------------------
# the format
# ------------------------------------------------------------------------------------------------------------------------
def quant(x, mutant=None):
    """x [..., Hkv, Dh] float32 holding T values -> (codes uint8 [..., Hkv, Dh], scale float32 [..., Hkv])."""
    x = np.asarray(x, dtype=np.float32)
    top = F32(240.0) if mutant == "max240" else E4M3_MAX
    a = np.abs(x)
    if mutant == "amax_half":
        a = a[..., : x.shape[-1] // 2]
    amax = a.max(axis=-1)
    if mutant == "per_token":
        amax = np.broadcast_to(amax.max(axis=-1, keepdims=True), amax.shape)
    s = (np.maximum(amax, AMAX_FLOOR) / top).astype(np.float32)
    with np.errstate(over="ignore"):
        y = x * (F32(1.0) / s)[..., None] if mutant == "recip" else x / s[..., None]
    y = np.clip(y.astype(np.float32), -top, top)
    return e4m3_encode(y, trunc=(mutant == "trunc")), np.ascontiguousarray(s)


def dequant(codes, scale, dtype):
    """-> float32 holding T(float(code) * s)."""
    return round_to(e4m3_decode(codes) * np.asarray(scale, dtype=np.float32)[..., None], dtype)


def cache_roundtrip(k, v, dtype, mutant=None):
    """What a store followed by the attention's staging makes of K / V [..., Hkv, Dh]: (k codes, k scales, v codes, v scales, the K the
    attention multiplies with, the V)."""
    kc, ks = quant(k, mutant)
    vc, vs = quant(v, mutant)
    return kc, ks, vc, vs, dequant(kc, ks, dtype), dequant(vc, ks if mutant == "k_scale_on_v" else vs, dtype)


# ------------------------------------------------------------------------------------------------------------------------
# needle rows
# ------------------------------------------------------------------------------------------------------------------------
def _tvalues(dtype, lo, hi):
    """every positive T value in [lo, hi]"""
    b = np.arange(1, 0x7C00 if dtype == "f16" else 0x7F80, dtype=np.uint32).astype(np.uint16)
    v = from_bits(b, dtype)
    return v[(v >= lo) & (v <= hi)]


def divide_needles(dtype, amax, count):
    """T values x <= amax whose code differs between x / s and x * (1 / s), s = amax / 448 (found by enumeration, ascending)."""
    s = F32(amax) / E4M3_MAX
    x = _tvalues(dtype, F32(amax) * F32(2.0 ** -12), F32(amax))
    a = e4m3_encode(np.clip(x / s, -448, 448))
    b = e4m3_encode(np.clip(x * (F32(1.0) / s), -448, 448))
    return x[a != b][:count]


def midpoint_values(dtype, amax):
    """T values that land exactly on the midpoint of two neighbouring codes after the division by s = amax / 448 (amax = 448 * 2^j: s
    is a power of two and the division exact), over the subnormal and the normal range."""
    s = F32(amax) / E4M3_MAX
    mids = (_POS[:-1] + _POS[1:]) / 2
    x = (mids * float(s)).astype(np.float32)
    keep = (round_to(x, dtype) == x) & (x.astype(np.float64) == mids * float(s)) & (x > 0)
    return x[keep]


_AMAX_TRIES = (3.0, 5.0, 6.5, 7.0, 11.0, 13.0, 0.8125, 1.375)


def needle_block(dtype, Hkv, Dh):
    """Tokens [n, Hkv, Dh] (float32 holding T values), one purpose each; head 0 carries the needle unless stated."""
    rng = np.random.default_rng(Dh + (0 if dtype == "f16" else 1))
    base = lambda: round_to(rng.standard_normal((Hkv, Dh)).astype(np.float32), dtype)
    rows, names = [], []

    t = base()                                    # heads 2^10 apart in magnitude
    for h in range(Hkv):
        t[h] = round_to(t[h] * F32(2.0 ** (-5 + 10 * (h % 2))), dtype)
    rows.append(t), names.append("heads-2^10-apart")

    t = round_to(base() * F32(0.125), dtype)      # the amax is the last column (and the largest of the first half is 2^-6 of it)
    t[:, Dh - 1] = F32(-24.0)
    rows.append(t), names.append("amax-last-column")

    t = np.zeros((Hkv, Dh), np.float32)           # code midpoints after an exact scaling: ties go to the even code
    m = midpoint_values(dtype, 448.0 * 2.0 ** -3)
    t[0, : min(len(m), Dh - 1)] = m[: Dh - 1] * np.where(np.arange(min(len(m), Dh - 1)) % 2, -1, 1).astype(np.float32)
    t[:, Dh - 1] = F32(448.0 * 2.0 ** -3)
    rows.append(t), names.append("midpoints")

    t = base()                                    # values whose code depends on dividing rather than multiplying by the reciprocal
    for amax in _AMAX_TRIES:
        d = divide_needles(dtype, amax, Dh - 1)
        if len(d):
            t[0] = 0
            t[0, : len(d)] = d
            t[0, Dh - 1] = F32(amax)
            break
    rows.append(t), names.append("divide")

    t = base()                                    # an all-zero row (and a row of negative zeros)
    t[0] = 0
    t[Hkv - 1] = F32(-0.0)
    rows.append(t), names.append("zero-row")

    t = round_to(base() * F32(2.0 ** -20), dtype)  # tiny rows: the scale is far below 1, subnormal T values appear for f16
    rows.append(t), names.append("tiny")

    if dtype == "f16":                            # the top of the f16 range
        t = round_to(base() * F32(1000.0), dtype)
        t[0, 1], t[0, Dh - 2] = F32(60000.0), F32(-60000.0)
        rows.append(t), names.append("f16-60000")
    return np.stack(rows), names


def random_block(dtype, n, Hkv, Dh, seed):
    """n tokens of N(0, 1) values, each (token, head) scaled by a power of two from 2^-6 .. 2^6"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, Hkv, Dh)).astype(np.float32)
    x *= (2.0 ** rng.integers(-6, 7, size=(n, Hkv, 1))).astype(np.float32)
    return round_to(x, dtype)


# ------------------------------------------------------------------------------------------------------------------------
# case lists of the GPU tests
# ------------------------------------------------------------------------------------------------------------------------
DTYPES = ("f16", "bf16")
STORE = dict(B=2, Bc=3, H=4, Hkv=2, lmax=160, S=(1, 5, 67), start=(0, 61), Dh=(64, 128))
STORE_CASES = [dict(S=S, Dh=Dh, dtype=dt, start=st) for S in STORE["S"] for Dh in STORE["Dh"] for dt in DTYPES for st in STORE["start"]]


def store_id(c):
    return f"S{c['S']}-Dh{c['Dh']}-{c['dtype']}-at{c['start']}"


def store_inputs(case):
    """qkv [B, S, (H + 2 Hkv) Dh] as float32 holding T values, freqs [S, B, Dh] float32, and `plain` [B, S] bool: tokens whose angles are
    all zero, so that the rotation leaves their q and k as they are (x * 1 + (+-y) * 0) and the K needles reach the quantiser.  Needle
    tokens fill the chunk from its start, in K and (another order) in V; the rest is random."""
    B, H, Hkv, S, Dh, dt = STORE["B"], STORE["H"], STORE["Hkv"], case["S"], case["Dh"], case["dtype"]
    rng = np.random.default_rng(S * 131 + Dh + case["start"])
    q = round_to(rng.standard_normal((B, S, H, Dh)).astype(np.float32), dt)
    k = random_block(dt, B * S, Hkv, Dh, seed=S + Dh).reshape(B, S, Hkv, Dh)
    v = random_block(dt, B * S, Hkv, Dh, seed=S + Dh + 1).reshape(B, S, Hkv, Dh)
    needles, _ = needle_block(dt, Hkv, Dh)
    freqs = (50.0 * rng.standard_normal((S, B, Dh))).astype(np.float32)
    plain = np.zeros((B, S), bool)
    for b in range(B):
        n = min(S, len(needles))
        order = (np.arange(n) + b * 3 + S) % len(needles)  # S = 1 still meets a different needle per batch row and case
        k[b, :n] = needles[order]
        v[b, :n] = needles[order[::-1]]
        plain[b, :n] = True
        freqs[:n, b] = 0
    qkv = np.concatenate([q.reshape(B, S, -1), k.reshape(B, S, -1), v.reshape(B, S, -1)], axis=-1)
    return qkv, freqs, plain, k, v


CHUNK = 64
SPLIT_FORCED = [dict(Sq=Sq, Sk=Sk, G=G, causal=c, Dh=Dh, dtype=dt) for Sk in (65, 130, 193) for Sq in (1, 8) for G in (1, 4)
                for c in (True, False) for Dh in (64, 128) for dt in DTYPES]
SPLIT_PLAN = [dict(Sq=Sq, Sk=Sk, G=4, causal=True, Dh=Dh, dtype=dt) for (Sq, Sk) in ((1, 2049), (4, 2111)) for Dh in (64, 128) for dt in DTYPES]
ONEPASS_TILES = (64, 128, 256)
ONEPASS_SHAPES = [(Sq, Sk, c) for Sq in (1, 33, 130) for Sk in (1, 63, 65, 193) for c in (True, False) if Sq <= Sk or not c]
ONEPASS = [dict(rows=r, Dh=Dh, dtype=dt) for r in ONEPASS_TILES for Dh in (64, 128) for dt in DTYPES]
ATTN_B, ATTN_HKV, ATTN_PAD = 2, 2, 3


def attn_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


_ATTN = {}


def attn_inputs(Sq, Sk, G, Dh, dtype):
    """q [B, Sq, H, Dh] (float32 holding T values, ~ 1.5 N) and an FP8 cache of Sk + ATTN_PAD rows: codes and scales of K ~ N and
    V ~ 1 + 0.5 N, every (key, head) scaled by a power of two from 2^-6 .. 2^6 so that a misindexed scale shows; the rows >= Sk hold
    the NaN code 0x7F and NaN scales so that a read past Sk shows.  Computed once per shape and shared (never written to)."""
    key = (Sq, Sk, G, Dh, dtype)
    if key not in _ATTN:
        B, Hkv = ATTN_B, ATTN_HKV
        rng = np.random.default_rng(Sq * 7919 + Sk * 31 + G + Dh)
        q = round_to(1.5 * rng.standard_normal((B, Sq, G * Hkv, Dh)).astype(np.float32), dtype)
        pw = lambda: (2.0 ** rng.integers(-6, 7, size=(B, Sk, Hkv, 1))).astype(np.float32)
        k = round_to(rng.standard_normal((B, Sk, Hkv, Dh)).astype(np.float32) * pw(), dtype)
        v = round_to((1 + 0.5 * rng.standard_normal((B, Sk, Hkv, Dh))).astype(np.float32) * pw(), dtype)
        L = Sk + ATTN_PAD
        kc, vc = np.full((B, L, Hkv, Dh), 0x7F, np.uint8), np.full((B, L, Hkv, Dh), 0x7F, np.uint8)
        ks, vs = np.full((B, L, Hkv), np.nan, np.float32), np.full((B, L, Hkv), np.nan, np.float32)
        kc[:, :Sk], ks[:, :Sk] = quant(k)
        vc[:, :Sk], vs[:, :Sk] = quant(v)
        _ATTN[key] = dict(q=q, k=k, v=v, kc=kc, ks=ks, vc=vc, vs=vs)
    return _ATTN[key]
