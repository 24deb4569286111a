"""The W8A8 family on the MI355X (csrc/awq_w8a8_cdna4.hip) against its restatements (tests/w8a8_oracle.py).  Every check runs through the
extension (the reference's five names) and through llm_awq_amd.ops (ctypes on the C ABI), and the two must give the same bits."""
import functools

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_oracle as A
from tests import w8a8_oracle as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
TILES = [64, 128]
# the smallest shapes that can go wrong: one MFMA step, partial row / column tiles of both tiles, more than one block, K tails, one whole-model shape
SHAPES = [(1, 16, 16), (63, 48, 80), (65, 272, 208), (129, 144, 1152), (300, 1152, 4304)]
# around the tiles the plan reports (tile_m -+ 1, tile_n -+ 8), with the K tails 32 and 48 (the shapes above all have K % 64 in {0, 16})
PLAN_SHAPES = [(63, 56, 96), (65, 72, 112), (127, 120, 96), (129, 136, 112)]
# ROCm documentation, "HIP math API" (ROCm 6.x / 7.x), table of single-precision functions: tanhf, maximum error 2 ULP.  2 ulp of a float
# is at most 2 * 2^-23 of its magnitude (tanh has no zero but at 0, where it is exact).  A larger documented bound would only enlarge the
# set of elements where either fp16 neighbour is accepted.
TANH_DELTA = 2.0 ** -22


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


@pytest.fixture
def tile():
    yield lambda t: _capi.tune(w8a8_tile=t)
    _capi.tune(w8a8_tile=0)


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype in (F16, torch.bfloat16) else t


def gemm_both(x, w, ws, as_, bias=None):
    """engine and ops on the same inputs -> out fp16 [M, N] (CPU); the two must agree bit for bit."""
    E = _engine()
    m, n = x.shape[0], w.shape[0]
    o1 = torch.full((m, n), float("nan"), dtype=F16, device=DEV)
    o2 = torch.full((m, n), float("nan"), dtype=F16, device=DEV)
    if bias is None:
        assert E.w8a8_gemm_forward_cuda(x, w, ws, as_, o1) is None
    else:
        assert E.w8a8_gemm_fuse_bias_forward_cuda(x, w, ws, as_, o1, bias) is None
    ops.w8a8_gemm(x, w, ws, as_, o2, bias)
    torch.cuda.synchronize()
    assert torch.equal(bits(o1), bits(o2))
    return o1.cpu()


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


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("t", TILES)
@pytest.mark.parametrize("m,n,k", SHAPES + PLAN_SHAPES)
def test_gemm_exact_lattice(tile, m, n, k, t, with_bias):
    c = lattice_case(m, n, k)
    tile(t)
    assert ops.w8a8_gemm_plan(m, n, k) == (-(-m // t) * -(-n // t), t, t)
    out = gemm_both(c["x"].to(DEV), c["w"].to(DEV), c["ws"].to(DEV), c["as_"].to(DEV), c["bias"].to(DEV) if with_bias else None)
    want = c["want"][with_bias]
    bad = bits(out) != bits(want)
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:4].tolist())


def test_plan_shapes_sit_around_the_reported_tiles(tile):
    for t in TILES:
        tile(t)
        _, tm, tn = ops.w8a8_gemm_plan(1000, 1000, 64)
        assert (tm, tn) == (t, t)
        assert (tm - 1, tn - 8) in [s[:2] for s in PLAN_SHAPES] and (tm + 1, tn + 8) in [s[:2] for s in PLAN_SHAPES]
    assert sorted({k % 64 for _, _, k in SHAPES + PLAN_SHAPES}) == [0, 16, 32, 48]


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("t", TILES)
@pytest.mark.parametrize("m,n,k", [(65, 272, 208), (300, 1152, 4304)])
def test_gemm_random_scales(tile, m, n, k, t, with_bias):
    """|out - e| <= 0.501 ulp_fp16(e) + 2^-22 (|acc ws as| + |bias|), e in float64: one rounding to fp16 plus the three fp32 roundings of the
    epilogue (int -> float, the two multiplies or multiply + fma: <= 3 * 2^-24 relative, and 2^-22 leaves room)."""
    g = torch.Generator().manual_seed(m + k)
    x = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8)
    w = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8)
    ws = (torch.rand(n, generator=g) * 0.004 + 0.0005).to(F16)  # |acc| ~ 74^2 sqrt(K) <= 4e5: outputs stay below ~100
    as_ = (torch.rand(m, generator=g) * 0.04 + 0.005).to(F16)
    bias = torch.randn(n, generator=g).to(F16) if with_bias else None
    tile(t)
    out = gemm_both(x.to(DEV), w.to(DEV), ws.to(DEV), as_.to(DEV), None if bias is None else bias.to(DEV))
    e, mag = W.gemm_f64(W.acc_exact(x, w), ws, as_, bias)
    assert torch.isfinite(out.float()).all()
    err, lim = (out.double() - e).abs(), 0.501 * A.ulp(e, F16) + 2.0 ** -22 * mag
    print(f"worst err / limit = {float((err / lim).max()):.4f}")
    assert not (err > lim).any(), (int((err > lim).sum()), float((err / lim).max()))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("t", TILES)
def test_gemm_saturation_needle(tile, t, with_bias):
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
    tile(t)
    out = gemm_both(x.to(DEV), w.to(DEV), ws.to(DEV), as_.to(DEV), None if bias is None else bias.to(DEV))
    want = W.gemm_f32(acc, ws, as_, bias).to(F16)
    assert float(want[0, 0]) == 67.25 and float(want[2, 16]) == 67.25 and float(want[0, 8]) == -66.75
    assert torch.equal(bits(out), bits(want)), (out[:, ::8], want[:, ::8])


@pytest.mark.parametrize("t", TILES)
def test_gemm_bounds(tile, t):
    """x and w inside larger buffers filled with 127, out inside a NaN buffer: a read past row M / N or column K would change the result, a
    write past the output would break the guard."""
    m, n, k = 65, 72, 208
    c = lattice_case(65, 272, 208)
    x, w, ws, as_, bias = c["x"], c["w"][:n].contiguous(), c["ws"][:n].contiguous(), c["as_"], c["bias"][:n].contiguous()
    tile(t)
    plain = gemm_both(x.to(DEV), w.to(DEV), ws.to(DEV), as_.to(DEV), bias.to(DEV))
    pad = 4096
    xb = torch.full((pad + m * k + pad,), 127, dtype=torch.int8, device=DEV)
    wb = torch.full((pad + n * k + pad,), 127, dtype=torch.int8, device=DEV)
    ob = torch.full((pad + m * n + pad,), float("nan"), dtype=F16, device=DEV)
    xv, wv, ov = xb[pad:pad + m * k].view(m, k), wb[pad:pad + n * k].view(n, k), ob[pad:pad + m * n].view(m, n)
    xv.copy_(x)
    wv.copy_(w)
    _engine().w8a8_gemm_fuse_bias_forward_cuda(xv, wv, ws.to(DEV), as_.to(DEV), ov, bias.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(ov.cpu()), bits(plain)) and torch.equal(bits(plain), bits(c["want"][True][:, :n]))
    assert torch.isnan(ob[:pad]).all() and torch.isnan(ob[pad + m * n:]).all()
    assert (xb[:pad] == 127).all() and (xb[pad + m * k:] == 127).all() and (wb[:pad] == 127).all() and (wb[pad + n * k:] == 127).all()


def check_gelu_stage(x, tmp, q, scale):
    """tmp: bit-exact wherever the fp16 rounding of tanh is decided (tanh(u) (1 -+ TANH_DELTA) round alike), else either neighbour;
    scale and q: bit-exact functions of the GPU's own tmp."""
    lo, hi = W.gelu_candidates(x.cpu(), TANH_DELTA)
    t = tmp.cpu()
    ok = (bits(t) == bits(lo)) | (bits(t) == bits(hi))
    assert ok.all(), (int((~ok).sum()), (~ok).nonzero()[:4].tolist())
    undecided = float((bits(lo) != bits(hi)).float().mean())
    assert undecided < 0.01, undecided  # the check is bit-exact on (nearly) every element
    qo, so = W.gelu_quant_from_tmp(t)
    assert torch.equal(bits(scale.cpu()), bits(so))
    assert torch.equal(q.cpu(), qo), int((q.cpu() != qo).sum())


def gelu_both(x):
    E = _engine()
    m, k = x.shape
    res = []
    for f in (E.gelu_and_quant, lambda q, xx, s, t: ops.gelu_quant_per_token(xx, q, s, t)):
        q = torch.full((m, k), 99, dtype=torch.int8, device=DEV)
        s = torch.full((m,), float("nan"), dtype=F16, device=DEV)
        tmp = torch.full((m, k), float("nan"), dtype=F16, device=DEV)
        assert f(q, x, s, tmp) is None
        res.append((tmp, q, s))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b))
    return res[0]


def test_determinism_and_capture_of_the_mlp(tile):
    """fc1 -> gelu_and_quant -> fc2 (QuantSiglipMLP's sequence, the scale buffer reused between the two GEMMs) eagerly, twice, and as a
    single-stream graph: equal bits; every stage is checked against its oracle fed with the GPU's previous stage."""
    E = _engine()
    m, hid, ffn = 65, 1152, 4304
    g = torch.Generator().manual_seed(7)
    w1 = torch.randint(-128, 128, (ffn, hid), generator=g, dtype=torch.int8).to(DEV)
    w2 = torch.randint(-128, 128, (hid, ffn), generator=g, dtype=torch.int8).to(DEV)
    ws1 = (torch.rand(ffn, generator=g) * 0.0004 + 0.0001).to(F16).to(DEV)
    ws2 = (torch.rand(hid, generator=g) * 0.0004 + 0.0001).to(F16).to(DEV)
    b1, b2 = (torch.randn(ffn, generator=g) * 0.1).to(F16).to(DEV), (torch.randn(hid, generator=g) * 0.1).to(F16).to(DEV)
    h = torch.randn(m, hid, generator=g).to(F16).to(DEV)
    xq = torch.empty(m, hid, dtype=torch.int8, device=DEV)
    aq = torch.empty(m, ffn, dtype=torch.int8, device=DEV)
    scale = torch.empty(m, dtype=F16, device=DEV)
    fc1, tmp = torch.empty(m, ffn, dtype=F16, device=DEV), torch.empty(m, ffn, dtype=F16, device=DEV)
    out = torch.empty(m, hid, dtype=F16, device=DEV)

    def run():
        E.invoke_quant(xq, h, scale)
        s0 = scale.clone()
        E.w8a8_gemm_fuse_bias_forward_cuda(xq, w1, ws1, scale, fc1, b1)
        E.gelu_and_quant(aq, fc1, scale, tmp)
        E.w8a8_gemm_fuse_bias_forward_cuda(aq, w2, ws2, scale, out, b2)
        return [t.clone() for t in (xq, s0, fc1, tmp, aq, scale, out)]

    first = run()
    second = run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up (allocator pools)
    torch.cuda.current_stream().wait_stream(s)
    for t in (xq, aq, scale, fc1, tmp, out):
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, captured):
        assert torch.equal(bits(a), bits(b))

    xq_, s0_, fc1_, tmp_, aq_, s1_, out_ = [t.cpu() for t in first]
    qo, so = W.quant_per_token(h)
    assert torch.equal(xq_, qo) and torch.equal(bits(s0_), bits(so))

    def within(o, x8, w8, ws, as_, b):
        e, mag = W.gemm_f64(W.acc_exact(x8, w8), ws, as_, b)
        err, lim = (o.double() - e).abs(), 0.501 * A.ulp(e, F16) + 2.0 ** -22 * mag
        assert torch.isfinite(o.float()).all() and not (err > lim).any(), float((err / lim).max())

    within(fc1_, xq_, w1.cpu(), ws1, s0_, b1)
    check_gelu_stage(fc1_, tmp_, aq_, s1_)
    within(out_, aq_, w2.cpu(), ws2, s1_, b2)


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [16, 80, 1152, 4304])
@pytest.mark.parametrize("m", [1, 130])
def test_invoke_quant(dtype, m, k):
    E = _engine()
    g = torch.Generator().manual_seed(100 * k + m)
    x = (torch.randn(m, k, generator=g) * 3).to(dtype)
    if m > 3:
        x[0] = 0                       # scale 0, q 0
        x[1] = -x[1].abs() - 0.5       # the row's maximum is negative
        x[2, 0], x[2, k - 1] = 65504.0, -65504.0
    xd = x.to(DEV)
    res = []
    for f in (E.invoke_quant, lambda q, xx, s: ops.quant_per_token(xx, q, s)):
        q = torch.full((m, k), 99, dtype=torch.int8, device=DEV)
        s = torch.full((m,), float("nan"), dtype=F16, device=DEV)
        assert f(q, xd, s) is None
        res.append((q.cpu(), s.cpu()))
    qo, so = W.quant_per_token(x)
    for q, s in res:
        assert torch.equal(bits(s), bits(so)), (s[:4], so[:4])
        assert torch.equal(q, qo), int((q != qo).sum())
    if m > 3:
        assert float(so[0]) == 0.0 and (qo[0] == 0).all() and int(qo[1].min()) == -127 and int(qo[1].max()) <= 0
        assert int(qo[2, 0]) == 127 and int(qo[2, k - 1]) == -127


def test_invoke_quant_refuses_float32():
    E = _engine()
    x = torch.zeros(2, 16, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        E.invoke_quant(torch.zeros(2, 16, dtype=torch.int8, device=DEV), x, torch.zeros(2, dtype=F16, device=DEV))
    with pytest.raises(TypeError, match="float16"):
        ops.quant_per_token(x, torch.zeros(2, 16, dtype=torch.int8, device=DEV), torch.zeros(2, dtype=F16, device=DEV))


@pytest.mark.parametrize("m,k", [(3, 80), (130, 4304)])
def test_gelu_and_quant_staged(m, k):
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(k + m)) * 2).to(F16)
    # the quirk (act.cu:45,52-54): positive values up to 1e-4 do not count towards amax.  Row 0: only such positives (gelu(1.5e-4) ~ 7.5e-5)
    # and zeros -> amax 0, scale 0.  Row 1: the same positives and small negatives (gelu(-4e-5) ~ -2e-5) -> amax comes from the negatives.
    x[0] = 0
    x[0, ::3] = 1.5e-4
    x[1] = -4e-5
    x[1, ::2] = 1.5e-4
    tmp, q, s = gelu_both(x.to(DEV))
    check_gelu_stage(x, tmp, q, s)
    t = tmp.cpu().float()
    assert 0 < float(t[0].max()) <= 1e-4 and float(s[0]) == 0.0
    assert 0 < float(t[1].max()) <= 1e-4 and float(t[1].min()) < 0 and 0 < float(s[1]) * 127 < 0.5 * float(t[1].max())


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [80, 1152, 4304])
@pytest.mark.parametrize("mode", ["token", "token_no_beta", "tensor"])
def test_rms_norm_general(dtype, k, mode):
    """|q - y64| <= 0.5 + 127 * 2^-10 + s and |scale - amax64 / 127| <= 0.5 ulp_fp16 + 2^-10 amax64 / 127, y64 = the float64 value with
    amax over T-rounded v.  s, the fp32 evaluation slack: mean and variance are blocked fp32 sums at most 72 additions deep, so each is
    within 72 * 2^-24 of sum |terms| / K, and with |mean| <= std (mean |x| <= 1.42 std) that moves (x - mean) rstd by at most
    ~2^-17 (|x - mean| / std + 1); the six elementwise roundings add 6 * 2^-24 relative.  Per element, in units of q:
    s = 2^-16 * mul * (|n gamma| + |beta| + |gamma|), mul = 127 / amax or scaling[0].
    token_no_beta: beta = None (the C entry's NULL, the binding's bias=None)."""
    E = _engine()
    m, eps = 37, 1e-6
    per_token = mode != "tensor"
    g = torch.Generator().manual_seed(10 * k + len(mode))
    std = torch.rand(m, 1, generator=g) * 2 + 0.5
    x = (torch.randn(m, k, generator=g) * std + (torch.rand(m, 1, generator=g) * 1.4 - 0.7) * std).to(dtype)
    gamma = (1 + 0.1 * torch.randn(k, generator=g)).to(dtype)
    beta = None if mode == "token_no_beta" else (0.1 * torch.randn(k, generator=g)).to(dtype)
    beta_d = None if beta is None else beta.to(DEV)
    scaling = torch.full((m,), 25.0, dtype=F16)
    xd = x.double()
    assert (xd.mean(-1).abs() <= xd.std(-1)).all()
    res = []
    for via_ops in (False, True):
        q = torch.full((m, k), 99, dtype=torch.int8, device=DEV)
        s = scaling.to(DEV).clone()
        if via_ops:
            ops.layernorm_quant(x.to(DEV), gamma.to(DEV), beta_d, s, q, eps, per_token)
        else:
            assert E.rms_norm_general(q, x.to(DEV), gamma.to(DEV), beta_d, s, eps, per_token) is None
        res.append((q.cpu(), s.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(bits(res[0][1]), bits(res[1][1]))
    q, s = res[0]
    y, amax, mag = W.layernorm_quant_f64(x, gamma, beta, eps, per_token, scaling)
    mul = (127.0 / amax)[:, None] if per_token else torch.full((m, 1), 25.0, dtype=torch.float64)
    slack = 2.0 ** -16 * mul * (mag + gamma.double().abs()[None, :])
    err = (q.double() - y.clamp(-128, 127)).abs()
    lim = 0.5 + 127 * 2.0 ** -10 + slack
    print(f"worst |q - y64| = {float(err.max()):.4f} (limit >= {float(lim.min()):.4f}), slack <= {float(slack.max()):.5f}")
    assert not (err > lim).any(), (int((err > lim).sum()), float(err.max()))
    if per_token:
        want = amax / 127.0
        serr = (s.double() - want).abs()
        assert not (serr > 0.5 * A.ulp(want, F16) + 2.0 ** -10 * want).any(), float(serr.max())
        assert int(q.abs().max()) == 127
    else:
        assert torch.equal(bits(s), bits(scaling))  # scaling is only read
        nobeta = torch.full((m, k), 99, dtype=torch.int8, device=DEV)
        E.rms_norm_general(nobeta, x.to(DEV), gamma.to(DEV), torch.zeros_like(beta).to(DEV), scaling.to(DEV), eps, False)
        assert torch.equal(nobeta.cpu(), q)  # beta is ignored in this mode (layernorm.cu:224-229)
