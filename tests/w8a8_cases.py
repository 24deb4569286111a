"""Inputs and acceptance criteria of the W8A8 checks, shared by tests/test_gpu_w8a8.py (the kernels) and tests/test_w8a8_host.py (the
restatements of tests/w8a8_oracle.py standing in for the kernels, unmutated and with one fault switched in).

Every criterion is a function of (what the kernel returned, the inputs) and returns its violations as a dict name -> count; an empty
dict passes.  The GPU tests assert exactly these, so a mutant the host tests see rejected here is rejected on the GPU as well.

    *_CHECKS            the list of checks the GPU suite runs per operation (dicts; `id` names one)
    *_inputs(check)     the tensors of one check, on the CPU
    *_stand_in(..)      the oracle's output in the kernel's place, with `mutant=` one fault
    mutant_applies      where the construction is bound to see a fault (reasons, not measurements)
"""
from __future__ import annotations

import functools

import torch

from tests import attn_oracle as A
from tests import w8a8_oracle as W

F16, BF16 = torch.float16, torch.bfloat16
TILES = [64, 128]
# the smallest shapes that can go wrong: one MFMA step, partial row / column tiles of both tiles, more than one block, K tails, one whole-model shape
SHAPES = [(1, 16, 16), (63, 48, 80), (65, 272, 208), (129, 144, 1152), (300, 1152, 4304)]
# around the tiles the plan reports (tile_m -+ 1, tile_n -+ 8), with the K tails 32 and 48 (the shapes above all have K % 64 in {0, 16})
PLAN_SHAPES = [(63, 56, 96), (65, 72, 112), (127, 120, 96), (129, 136, 112)]
RANDOM_SHAPES = [(65, 272, 208), (300, 1152, 4304)]
# ROCm documentation, "HIP math API" (ROCm 6.x / 7.x), table of single-precision functions: tanhf, maximum error 2 ULP.  2 ulp of a float
# is at most 2 * 2^-23 of its magnitude (tanh has no zero but at 0, where it is exact).  A larger documented bound would only enlarge the
# set of elements where either fp16 neighbour is accepted.
TANH_DELTA = 2.0 ** -22


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype in (F16, BF16) else t


def _name(dtype):
    return str(dtype)[6:]


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_case(m, n, k):
    """int8 inputs in [-7, 7], power-of-two scales, bias on the lattice 2^-10: every fp32 step of the epilogue is exact
    (|acc| < 2^18, acc ws as is a multiple of 2^-13 below 2^8, bias a multiple of 2^-10 below 4: 22 bits)."""
    g = torch.Generator().manual_seed(1000 * m + 10 * n + k)
    x = torch.randint(-7, 8, (m, k), generator=g, dtype=torch.int8)
    w = torch.randint(-7, 8, (n, k), generator=g, dtype=torch.int8)
    ws = torch.pow(2.0, -torch.randint(7, 10, (n,), generator=g).float()).to(F16)
    as_ = torch.pow(2.0, -torch.randint(3, 5, (m,), generator=g).float()).to(F16)
    bias = (torch.randint(-4095, 4096, (n,), generator=g).float() * 2.0 ** -10).to(F16)
    acc = W.acc_exact(x, w)
    want = {}
    for b in (None, bias):
        e, _ = W.gemm_f64(acc, ws, as_, b)
        assert torch.equal(e, W.gemm_f32(acc, ws, as_, b).double())  # the fp32 arithmetic is exact on this lattice
        want[b is not None] = e.to(torch.float32).to(F16)
    return dict(x=x, w=w, ws=ws, as_=as_, bias=bias, want=want)


@functools.lru_cache(maxsize=None)
def random_case(m, n, k, with_bias):
    """Full-range int8 operands and scales with full mantissas: the roundings of the epilogue are all in play."""
    g = torch.Generator().manual_seed(m + k)
    x = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8)
    w = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8)
    ws = (torch.rand(n, generator=g) * 0.004 + 0.0005).to(F16)  # |acc| ~ 74^2 sqrt(K) <= 4e5: outputs stay below ~100
    as_ = (torch.rand(m, generator=g) * 0.04 + 0.005).to(F16)
    bias = torch.randn(n, generator=g).to(F16) if with_bias else None
    return dict(x=x, w=w, ws=ws, as_=as_, bias=bias)


@functools.lru_cache(maxsize=None)
def needle_case(with_bias):
    """K = 4304 with x = -128: against w = -128 the sum is 70 516 736 > 2^24, against w = 127 it is -69 965 824.  Row 2 of x and column 16
    of w add a sum that is NOT a float: 70 483 965 = 2151 * 2^15 - 3.  float(acc) (nearest-even) is 2151 * 2^15, which times 2^-20 is a
    tie of fp16 and rounds to even, 67.25; a truncating conversion (.. - 8) or an exact evaluation (.. - 3) would give 67.1875."""
    k, n = 4304, 24
    x = torch.full((3, k), -128, dtype=torch.int8)
    w = torch.full((n, k), -128, dtype=torch.int8)
    w[8:16] = 127
    x[2, 0], x[2, -1] = 0, -3
    w[16:, -1] = 1
    acc = W.acc_exact(x, w)
    assert int(acc[0, 0]) == 70516736 and int(acc[0, 8]) == -69965824 and int(acc[2, 16]) == 70483965
    ws = torch.full((n,), 2.0 ** -14, dtype=F16)
    as_ = torch.full((3,), 2.0 ** -6, dtype=F16)
    bias = torch.zeros(n, dtype=F16) if with_bias else None
    want = W.gemm_f32(acc, ws, as_, bias).to(F16)
    assert float(want[0, 0]) == 67.25 and float(want[2, 16]) == 67.25 and float(want[0, 8]) == -66.75
    return dict(x=x, w=w, ws=ws, as_=as_, bias=bias, want=want)


@functools.lru_cache(maxsize=None)
def bounds_case(with_bias):
    """The lattice case (65, 272, 208) cut to 72 columns: one whole and one partial column tile of 64, a partial one of 128."""
    n = 72
    c = lattice_case(65, 272, 208)
    return dict(x=c["x"], w=c["w"][:n].contiguous(), ws=c["ws"][:n].contiguous(), as_=c["as_"], bias=c["bias"][:n].contiguous() if with_bias else None,
                want=c["want"][with_bias][:, :n].contiguous())


def _gemm_checks():
    out = []
    for b in (False, True):
        tag = "bias" if b else "nobias"
        for m, n, k in SHAPES + PLAN_SHAPES:
            out.append(dict(id=f"lattice-{m}x{n}x{k}-{tag}", kind="lattice", m=m, n=n, k=k, with_bias=b))
        for m, n, k in RANDOM_SHAPES:
            out.append(dict(id=f"random-{m}x{n}x{k}-{tag}", kind="random", m=m, n=n, k=k, with_bias=b))
            out.append(dict(id=f"exact-{m}x{n}x{k}-{tag}", kind="exact", m=m, n=n, k=k, with_bias=b))
        out.append(dict(id=f"needle-{tag}", kind="needle", m=3, n=24, k=4304, with_bias=b))
        out.append(dict(id=f"bounds-{tag}", kind="bounds", m=65, n=72, k=208, with_bias=b))
    return out


GEMM_CHECKS = _gemm_checks()


def gemm_inputs(check):
    """-> dict(x, w, ws, as_, bias (None without), want (fp16, where the check is bit-exact))."""
    kind, b = check["kind"], check["with_bias"]
    if kind == "lattice":
        c = lattice_case(check["m"], check["n"], check["k"])
        return dict(c, bias=c["bias"] if b else None, want=c["want"][b])
    if kind == "needle":
        return needle_case(b)
    if kind == "bounds":
        return bounds_case(b)
    c = random_case(check["m"], check["n"], check["k"], b)
    return dict(c, want=gemm_stand_in(c)) if kind == "exact" else c


_ACC = {}


def _acc(c, droptail=False):
    """The int32 sums of the inputs c, computed once."""
    key = (id(c["x"]), id(c["w"]), droptail)
    if key not in _ACC:
        _ACC[key] = (c["x"], c["w"], W.acc_exact(c["x"], c["w"], "droptail" if droptail else None))  # (holding x and w keeps their ids alive)
    return _ACC[key][2]


def gemm_stand_in(c, mutant=None):
    """The specification's output for the inputs c (fp16 [M, N])."""
    return W.gemm_f32(_acc(c, mutant == "droptail"), c["ws"], c["as_"], c["bias"], mutant).to(F16)


def gemm_bits(out, c):
    """out == want, bit for bit, no exclusions."""
    bad = bits(out) != bits(c["want"])
    return {"bits": int(bad.sum()), "first": bad.nonzero()[:4].tolist()} if bad.any() else {}


def gemm_bound(out, c):
    """|out - e| <= 0.501 ulp_fp16(e) + 2^-22 (|acc ws as| + |bias|), e in float64: one rounding to fp16 plus the three fp32 roundings of the
    epilogue (int -> float, the two multiplies or multiply + fma: <= 3 * 2^-24 relative, and 2^-22 leaves room)."""
    e, mag = W.gemm_f64(_acc(c), c["ws"], c["as_"], c["bias"])
    v = {}
    if not torch.isfinite(out.float()).all():
        v["finite"] = int((~torch.isfinite(out.float())).sum())
    err, lim = (out.double() - e).abs(), 0.501 * A.ulp(e, F16) + 2.0 ** -22 * mag
    print(f"worst err / limit = {float((err / lim).max()):.4f}")
    if (err > lim).any():
        v["bound"] = int((err > lim).sum())
        v["worst"] = float((err / lim).max())
    return v


def gemm_criterion(check):
    return gemm_bound if check["kind"] == "random" else gemm_bits


def gemm_mutant_applies(check, mutant) -> bool:
    kind, b = check["kind"], check["with_bias"]
    if mutant == "droptail":    # the tail columns hold data in every case
        return check["k"] % 64 != 0
    if mutant == "bias_first":  # moves the result by bias (1 - as); the needle's bias is zero
        return b and kind != "needle"
    if mutant == "trunc":       # float(acc) is exact up to 2^24, which only the needle's sums pass
        return kind == "needle"
    if mutant == "exact":       # differs through the rounding of t = float(acc) ws on the bias path.  (On the needle the exact value rounded
        # to fp32 IS float(acc) 2^-20, the scales being powers of two: only a direct rounding to fp16 would differ, which `trunc` stands for)
        return b and kind == "exact" and check["m"] * check["n"] >= 300 * 1152
    # one or two fp32 roundings more or fewer: a few fp16 results in 10^5 change, so only a bit-exact check of many elements sees them
    if mutant == "assoc":
        return (not b) and kind == "exact" and check["m"] * check["n"] >= 300 * 1152
    if mutant in ("nofma", "assoc_bias"):
        return b and kind == "exact" and check["m"] * check["n"] >= 300 * 1152
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# invoke_quant
# ------------------------------------------------------------------------------------------------------------------------
TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 125.5, -126.5, 3.5, -3.5, 4.5, -4.5, 0.0, 1.0, -1.0]
TIES_Q = [0, 0, 2, -2, 2, -2, 126, -126, 4, -4, 4, -4, 0, 1, -1]  # nearest-even


def quant_inputs(dtype, m, k):
    g = torch.Generator().manual_seed(100 * k + m)
    x = (torch.randn(m, k, generator=g) * 3).to(dtype)
    if m > 3:
        x[0] = 0                       # scale 0, q 0
        x[1] = -x[1].abs() - 0.5       # the row's maximum is negative
        x[2, 0], x[2, k - 1] = 65504.0, -65504.0
    return x


def quant_needle(dtype, k):
    """-> (x [5, k], q_want [5, k], scale_want [5]).  Rows 0-2, ties: one +-127 makes 127 / amax exactly 1 and the scale exactly 1.0, every
    other element is a half-integer (exact in fp16 and bf16), so q is the conversion's rounding of a tie and nothing else.  Rows 3-4,
    one +-inf among finite values: the scale is inf, 127 / inf = 0, finite * 0 = 0 and inf * 0 = NaN -> 0."""
    reps = -(-k // len(TIES))
    t = torch.tensor((TIES * reps)[:k])
    tq = torch.tensor((TIES_Q * reps)[:k], dtype=torch.int8)
    x = torch.stack([t, t, t, t, t]).clone()
    q = torch.stack([tq, tq, tq, torch.zeros_like(tq), torch.zeros_like(tq)]).clone()
    x[0, 0], x[1, k - 1], x[2, k // 2] = 127.0, 127.0, -127.0
    q[0, 0], q[1, k - 1], q[2, k // 2] = 127, 127, -127
    x[3, 3], x[4, k - 2] = float("inf"), float("-inf")
    xt = x.to(dtype)
    assert torch.equal(xt.float(), x)
    inf = float("inf")
    return xt, q, torch.tensor([1.0, 1.0, 1.0, inf, inf], dtype=F16)


def _quant_checks():
    out = []
    for dtype in (F16, BF16):
        for k in (16, 80, 1152, 4304):
            for m in (1, 130):
                out.append(dict(id=f"random-{_name(dtype)}-{m}x{k}", kind="random", dtype=dtype, m=m, k=k))
        for k in (16, 80):
            out.append(dict(id=f"needle-{_name(dtype)}-{k}", kind="needle", dtype=dtype, m=5, k=k))
            out.append(dict(id=f"leading-{_name(dtype)}-{k}", kind="leading", dtype=dtype, m=38, k=k))
    return out


QUANT_CHECKS = _quant_checks()


def quant_check_inputs(check):
    if check["kind"] == "needle":
        return quant_needle(check["dtype"], check["k"])[0]
    x = quant_inputs(check["dtype"], check["m"], check["k"])
    return x.reshape(2, 19, check["k"]) if check["kind"] == "leading" else x


def quant_stand_in(x, mutant=None):
    return W.quant_per_token(x, mutant)


def quant_bits(q, s, x):
    """q and scale equal the restatement's, bit for bit."""
    qo, so = W.quant_per_token(x)
    q, s = q.reshape(qo.shape), s.reshape(-1)[:so.numel()]
    v = {}
    if not torch.equal(bits(s), bits(so)):
        v["scale"] = int((bits(s) != bits(so)).sum())
    if not torch.equal(q, qo):
        v["q"] = int((q != qo).sum())
    return v


def quant_mutant_applies(check, mutant) -> bool:
    if mutant == "half_away":       # random products do not land on x.5: only the ties do
        return check["kind"] == "needle"
    if mutant == "trunc":           # half of all random products have a fraction above .5; the ties 1.5, 2.5 .. truncate differently as well
        return True
    if mutant == "inv_from_scale":
        # the inverse moves by up to 2^-11 relative and q by up to 127 * 2^-11 = 0.06: about 3 % of the elements of a random row change, so
        # a thousand elements are bound to show it; the needles' scales (1 and inf) invert exactly
        return check["kind"] != "needle" and check["m"] * check["k"] >= 1152
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# gelu_and_quant
# ------------------------------------------------------------------------------------------------------------------------
def gelu_inputs(m, k):
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(k + m)) * 2).to(F16)
    # the quirk (act.cu:45,52-54): positive values up to 1e-4 do not count towards amax.  Row 0: only such positives (gelu(1.5e-4) ~ 7.5e-5)
    # and zeros -> amax 0, scale 0.  Row 1: the same positives and small negatives (gelu(-4e-5) ~ -2e-5) -> amax comes from the negatives.
    x[0] = 0
    x[0, ::3] = 1.5e-4
    x[1] = -4e-5
    x[1, ::2] = 1.5e-4
    return x


OVERFLOW = [1500.0, -1500.0, 30000.0, -30000.0, 65504.0, -65504.0]


def gelu_overflow_inputs():
    """-> (x [6, 80], big: the mask of the planted values).  Above |x| ~ 1210 the fp16 product (0.044715h x) x overflows to inf, so
    u = +-inf, tanh = +-1 exactly and g = 0.5 x * 2 = x for positive x, 0.5 x * 0 = -0 for negative x.  Row r holds OVERFLOW[r] at every
    seventh column from r, the opposite sign once, and ordinary values elsewhere."""
    m, k = len(OVERFLOW), 80
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(1210)) * 2).to(F16)
    big = torch.zeros(m, k, dtype=torch.bool)
    for r, val in enumerate(OVERFLOW):
        x[r, r::7] = val
        x[r, r + 7] = -val
        big[r, r::7] = True
    assert (x[big].abs() >= 1500).all() and (x[~big].abs() < 16).all()
    return x, big


def _gelu_checks():
    return [dict(id="staged-3x80", kind="staged", m=3, k=80), dict(id="staged-130x4304", kind="staged", m=130, k=4304),
            dict(id="overflow", kind="overflow", m=6, k=80), dict(id="leading-38x16", kind="leading", m=38, k=16),
            dict(id="leading-38x80", kind="leading", m=38, k=80)]


GELU_CHECKS = _gelu_checks()


def gelu_check_inputs(check):
    if check["kind"] == "overflow":
        return gelu_overflow_inputs()[0]
    x = gelu_inputs(check["m"], check["k"])
    return x.reshape(2, 19, check["k"]) if check["kind"] == "leading" else x


def gelu_stand_in(x, mutant=None, hi=False):
    """-> (tmp, q, scale): either candidate of the GELU, then the quantisation of that tmp."""
    tmp = W.gelu_candidates(x, TANH_DELTA, mutant if mutant == "single_rounding" else None)[int(hi)]
    q, s = W.gelu_quant_from_tmp(tmp, None if mutant == "single_rounding" else mutant)
    return tmp, q, s


def check_gelu_stage(x, tmp, q, scale):
    """tmp: bit-exact wherever the fp16 rounding of tanh is decided (tanh(u) (1 -+ TANH_DELTA) round alike), else either neighbour;
    scale and q: bit-exact functions of the kernel's own tmp.  The undecided share stays below 1 %."""
    lo, hi = W.gelu_candidates(x.cpu(), TANH_DELTA)
    t = tmp.cpu().reshape(lo.shape)
    v = {}
    ok = (bits(t) == bits(lo)) | (bits(t) == bits(hi))
    if not ok.all():
        v["tmp"] = int((~ok).sum())
        v["first"] = (~ok).nonzero()[:4].tolist()
    undecided = float((bits(lo) != bits(hi)).float().mean())
    if not undecided < 0.01:  # the check is bit-exact on (nearly) every element
        v["undecided"] = undecided
    qo, so = W.gelu_quant_from_tmp(t)
    s, qq = scale.cpu().reshape(-1)[:so.numel()], q.cpu().reshape(qo.shape)
    if not torch.equal(bits(s), bits(so)):
        v["scale"] = int((bits(s) != bits(so)).sum())
    if not torch.equal(qq, qo):
        v["q"] = int((qq != qo).sum())
    return v


def gelu_mutant_applies(check, mutant) -> bool:
    if mutant == "single_rounding":  # the fp16 chain loses up to several ulp against one rounding, on random values and on -0 / x alike
        return check["kind"] != "overflow"   # .. but the overflow rows give x and 0 either way (only the sign of zero differs: not relied on)
    if mutant == "plain_abs":        # rows 0 and 1 of gelu_inputs hold positives below 1e-4 that must not count
        return check["kind"] in ("staged", "leading")
    if mutant in ("prod_f32", "inv_f32"):  # a rounding to fp16 (2^-11 relative) of values up to 127 moves about 3 % of random elements
        return check["kind"] != "overflow" and check["m"] * check["k"] >= 1152
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# rms_norm_general
# ------------------------------------------------------------------------------------------------------------------------
LN_MAX_K = 16384
DEPTH = 72        # the depth the bound's slack was written for (K <= 4304)
DEPTH_16384 = 73  # K = 16384: 8 vectors x 8 elements per thread (64 additions), 6 shuffle steps, 3 additions across the four waves


def ln_inputs(dtype, k, mode, m=37, eps=1e-6, std_scale=1.0, scaling=None):
    """Rows with std in [0.5, 2.5] * std_scale and a mean within 0.7 std; gamma around 1, beta around 0 (None for token_no_beta)."""
    g = torch.Generator().manual_seed(10 * k + len(mode))
    std = torch.rand(m, 1, generator=g) * 2 + 0.5
    x = torch.randn(m, k, generator=g) * std + (torch.rand(m, 1, generator=g) * 1.4 - 0.7) * std
    x = (x if std_scale == 1.0 else x * std_scale).to(dtype)
    gamma = (1 + 0.1 * torch.randn(k, generator=g)).to(dtype)
    beta = None if mode == "token_no_beta" else (0.1 * torch.randn(k, generator=g)).to(dtype)
    if scaling is None:
        scaling = torch.full((m,), 25.0, dtype=F16)
    xd = x.double()
    assert (xd.mean(-1).abs() <= xd.std(-1)).all()  # the bound's derivation needs |mean| <= std
    return dict(x=x, gamma=gamma, beta=beta, scaling=scaling, eps=eps, per_token=mode != "tensor", mode=mode, depth=DEPTH)


def _ln_checks():
    out = []
    for dtype in (F16, BF16):
        d = _name(dtype)
        for k in (80, 1152, 4304):
            for mode in ("token", "token_no_beta", "tensor"):
                out.append(dict(id=f"general-{d}-{k}-{mode}", kind="general", dtype=dtype, k=k, mode=mode))
        for k in (80, 1152):
            out.append(dict(id=f"eps-small-std-{d}-{k}-token", kind="eps_small", dtype=dtype, k=k, mode="token"))
            out.append(dict(id=f"eps-small-std-{d}-{k}-tensor", kind="eps_small", dtype=dtype, k=k, mode="tensor"))
            out.append(dict(id=f"eps-1e-2-{d}-{k}-token", kind="eps_big", dtype=dtype, k=k, mode="token"))
        out.append(dict(id=f"scaling-{d}-80", kind="scaling", dtype=dtype, k=80, mode="tensor"))
        for k in (8, 2048, 2056, 16376, 16384):
            out.append(dict(id=f"depth-{d}-{k}", kind="depth", dtype=dtype, k=k, mode="token"))
        out.append(dict(id=f"leading-{d}-80", kind="leading", dtype=dtype, k=80, mode="token"))
    return out


LN_CHECKS = _ln_checks()


def ln_check_inputs(check):
    dtype, k, mode, kind = check["dtype"], check["k"], check["mode"], check["kind"]
    if kind == "general":
        return ln_inputs(dtype, k, mode)
    if kind == "eps_small":   # var ~ 2.5e-7 .. 6e-6 against eps = 1e-6
        return ln_inputs(dtype, k, mode, std_scale=1e-3)
    if kind == "eps_big":     # var 0.25 .. 6 against eps = 1e-2
        return ln_inputs(dtype, k, mode, eps=1e-2)
    if kind == "scaling":     # per tensor: only element 0 counts
        s = torch.arange(1, 38, dtype=torch.float32) + 1
        s[0] = 25.0
        return ln_inputs(dtype, k, mode, scaling=s.to(F16))
    if kind == "depth":       # one to eight register vectors per thread
        return dict(ln_inputs(dtype, k, mode, m=3), depth=DEPTH_16384)
    if kind == "leading":
        c = ln_inputs(dtype, k, mode, m=38)
        return dict(c, x=c["x"].reshape(2, 19, k))
    raise ValueError(kind)


def ln_stand_in(c, mutant=None):
    """-> (q, scale): the nearest integer of the float64 value, the fp16 rounding of amax / 127 (per tensor: scaling as it came)."""
    y, amax, _ = W.layernorm_quant_f64(c["x"], c["gamma"], c["beta"], c["eps"], c["per_token"], c["scaling"], mutant)
    q = torch.round(y.clamp(-128, 127)).to(torch.int8)
    return q, ((amax / 127.0).to(torch.float32).to(F16) if c["per_token"] else c["scaling"].clone())


def ln_bound(q, s, c):
    """|q - y64| <= 0.5 + 127 * 2^-10 + sl and |scale - amax64 / 127| <= 0.5 ulp_fp16 + 2^-10 amax64 / 127, y64 = the float64 value with
    amax over T-rounded v.  sl, the fp32 evaluation slack: mean and variance are blocked fp32 sums at most `depth` = 72 additions deep, so
    each is within 72 * 2^-24 of sum |terms| / K, and with |mean| <= std (mean |x| <= 1.42 std) that moves (x - mean) rstd by at most
    ~2^-17 (|x - mean| / std + 1); the six elementwise roundings add 6 * 2^-24 relative.  Per element, in units of q:
    sl = (depth / 72) 2^-16 * mul * (|n gamma| + |beta| + |gamma|), mul = 127 / amax or scaling[0].  A larger var + eps only shrinks these.
    Per token the row's peak is 127 in magnitude; per tensor scaling comes back unchanged."""
    q, s = q.cpu(), s.cpu()
    y, amax, mag = W.layernorm_quant_f64(c["x"], c["gamma"], c["beta"], c["eps"], c["per_token"], c["scaling"])
    q = q.reshape(y.shape)
    mul = (127.0 / amax)[:, None] if c["per_token"] else torch.full((y.shape[0], 1), float(c["scaling"][0]), dtype=torch.float64)
    slack = c["depth"] / DEPTH * 2.0 ** -16 * mul * (mag + c["gamma"].double().abs()[None, :])
    err = (q.double() - y.clamp(-128, 127)).abs()
    lim = 0.5 + 127 * 2.0 ** -10 + slack
    print(f"worst |q - y64| = {float(err.max()):.4f} (limit >= {float(lim.min()):.4f}), worst err / limit = {float((err / lim).max()):.4f}, "
          f"slack <= {float(slack.max()):.5f}")
    v = {}
    if (err > lim).any():
        v["q"] = int((err > lim).sum())
        v["worst"] = float(err.max())
    if c["per_token"]:
        want = amax / 127.0
        serr, slim = (s.double().reshape(-1)[:want.numel()] - want).abs(), 0.5 * A.ulp(want, F16) + 2.0 ** -10 * want
        print(f"worst scale err / limit = {float((serr / slim).max()):.4f}")
        if (serr > slim).any():
            v["scale"] = int((serr > slim).sum())
        if int(q.abs().max()) != 127:
            v["peak"] = int(q.abs().max())
    elif not torch.equal(bits(s), bits(c["scaling"])):  # scaling is only read
        v["scaling"] = int((bits(s) != bits(c["scaling"])).sum())
    return v


def ln_mutant_applies(check, mutant) -> bool:
    kind, mode, k = check["kind"], check["mode"], check["k"]
    if mutant in ("noeps", "eps_outside"):  # eps must weigh against var: 1e-6 against std ~ 1e-3, or 1e-2 against std ~ 1
        return kind in ("eps_small", "eps_big")
    if mutant == "rms":             # the rows' means are up to 0.7 std: q moves by up to 127 * 0.7 / max |n|
        c = ln_check_inputs(check)
        xd = c["x"].double().reshape(-1, k)
        return bool(((xd.mean(-1).abs() / xd.std(-1)) > 0.1).any())
    if mutant == "unbiased":        # 1 / (2 K) relative: 0.6 % at K = 80 (0.8 in q at the peak, against 0.62), 0.04 % at K = 1152
        return k <= 80
    if mutant == "amax_unrounded":  # the peak's rounding to T moves the scale by up to 2^-9 relative in bf16 (2^-12 in fp16) against a tolerance
        # of at most 2^-10 + 2^-11: about one bf16 row in four passes it, so 37 rows are bound to (3 rows are not); per tensor no amax
        return check["dtype"] == BF16 and mode != "tensor" and kind != "depth"
    if mutant == "scale_row":
        return kind == "scaling"
    if mutant in ("beta_tensor", "scale_divides"):
        return mode == "tensor"
    if mutant == "nobeta_token":
        return mode == "token"
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# the two staged sequences of a tower layer
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mlp_inputs():
    """fc1 -> gelu_and_quant -> fc2 at SigLIP's sizes, 65 tokens."""
    m, hid, ffn = 65, 1152, 4304
    g = torch.Generator().manual_seed(7)
    w1 = torch.randint(-128, 128, (ffn, hid), generator=g, dtype=torch.int8)
    w2 = torch.randint(-128, 128, (hid, ffn), generator=g, dtype=torch.int8)
    ws1 = (torch.rand(ffn, generator=g) * 0.0004 + 0.0001).to(F16)
    ws2 = (torch.rand(hid, generator=g) * 0.0004 + 0.0001).to(F16)
    b1, b2 = (torch.randn(ffn, generator=g) * 0.1).to(F16), (torch.randn(hid, generator=g) * 0.1).to(F16)
    h = torch.randn(m, hid, generator=g).to(F16)
    return dict(m=m, hid=hid, ffn=ffn, w1=w1, w2=w2, ws1=ws1, ws2=ws2, b1=b1, b2=b2, h=h)


@functools.lru_cache(maxsize=None)
def layer_inputs():
    """The attention half: E = 256, 4 heads of 64, 2 x 70 tokens, fp16."""
    bsz, seqlen, heads, dh = 2, 70, 4, 64
    emb, m = heads * dh, bsz * seqlen
    ln = ln_inputs(F16, emb, "token", m=m)
    g = torch.Generator().manual_seed(256)
    wqkv = torch.randint(-128, 128, (3 * emb, emb), generator=g, dtype=torch.int8)
    wo = torch.randint(-128, 128, (emb, emb), generator=g, dtype=torch.int8)
    ws_qkv = (torch.rand(3 * emb, generator=g) * 0.0008 + 0.0004).to(F16)  # |acc| ~ 40 * 74 * 16, ascale ~ 0.03: q, k, v of order 1
    ws_o = (torch.rand(emb, generator=g) * 0.0008 + 0.0004).to(F16)
    b_qkv, b_o = (torch.randn(3 * emb, generator=g) * 0.1).to(F16), (torch.randn(emb, generator=g) * 0.1).to(F16)
    return dict(bsz=bsz, seqlen=seqlen, heads=heads, dh=dh, emb=emb, m=m, ln=ln, wqkv=wqkv, wo=wo, ws_qkv=ws_qkv, ws_o=ws_o, b_qkv=b_qkv, b_o=b_o)


def gemm_stage(out, x, w, ws, as_, bias):
    """One GEMM of a sequence against the specified epilogue on the previous stage's output, bit for bit."""
    c = dict(x=x, w=w, ws=ws, as_=as_, bias=bias)
    return gemm_bits(out, dict(c, want=gemm_stand_in(c)))


def attention_stage(attn, qkv, L):
    """flash_attn_func(causal=False) on the q / k / v views of qkv [m, 3 E] within the prefill attention bound (tests/attn_prefill_oracle.py)."""
    from tests import attn_prefill_oracle as O

    shape = (L["bsz"], L["seqlen"], L["heads"], L["dh"])
    q, k, v = [t.reshape(shape) for t in qkv.split(L["emb"], dim=-1)]
    ref, Aw, qk = O.attention(q, k, v, None, False, stats=True)
    lim = O.bound(ref, Aw, qk, F16, L["seqlen"], L["dh"], L["dh"] ** -0.5)
    err = (attn.reshape(shape).double() - ref).abs()
    print(f"attention: max err / bound = {float((err / lim).max()):.3f}")
    out = {}
    if not torch.isfinite(attn.float()).all():
        out["finite"] = int((~torch.isfinite(attn.float())).sum())
    if (err > lim).any():
        out["bound"] = int((err > lim).sum())
    if not (float(qkv.float().std()) > 0.3 and float(ref.std()) > 0.05):  # the stages carry signal
        out["signal"] = (float(qkv.float().std()), float(ref.std()))
    return out
