"""The W8A8 family on the MI355X (csrc/awq_w8a8_cdna4.hip) against its restatements (tests/w8a8_oracle.py).  Every check runs through the
extension (the reference's five names) and through llm_awq_amd.ops (ctypes on the C ABI), and the two must give the same bits.  The inputs
and the acceptance criteria live in tests/w8a8_cases.py; tests/test_w8a8_host.py proves on the CPU that each criterion passes the
restatement and rejects it with any one applicable fault (w8a8_oracle's mutants) switched in."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.w8a8_linear import W8A8OF16LinearDynamicInputScale
from tests import w8a8_cases as C
from tests import w8a8_oracle as W
from tests.w8a8_cases import PLAN_SHAPES, SHAPES, TILES, bits, lattice_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def _flash():
    llm_awq_amd.install_as_flash_attn()
    from flash_attn import flash_attn_func  # the name the towers import

    return flash_attn_func


@pytest.fixture
def tile():
    yield lambda t: _capi.tune(w8a8_tile=t)
    _capi.tune(w8a8_tile=0)


def _dev(t):
    return None if t is None else t.to(DEV)


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


def gemm_case(c):
    return gemm_both(c["x"].to(DEV), c["w"].to(DEV), c["ws"].to(DEV), c["as_"].to(DEV), _dev(c["bias"]))


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
@pytest.mark.parametrize("m,n,k", C.RANDOM_SHAPES)
def test_gemm_random_scales(tile, m, n, k, t, with_bias):
    """|out - e| <= 0.501 ulp_fp16(e) + 2^-22 (|acc ws as| + |bias|), e in float64 (C.gemm_bound)."""
    c = C.random_case(m, n, k, with_bias)
    tile(t)
    v = C.gemm_bound(gemm_case(c), c)
    assert not v, v


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("t", TILES)
@pytest.mark.parametrize("m,n,k", C.RANDOM_SHAPES)
def test_gemm_random_scales_bit_exact(tile, m, n, k, t, with_bias):
    """The same inputs against the specified fp32 epilogue, bit for bit and with no exclusions: the accumulator is an exact int32 and every
    later step (int -> float, the multiplies, the fma, the rounding to fp16) is one IEEE operation with contraction off, so the
    association the kernel's header promises is observable.  Of the large case's 345 600 results, 8 to 17 change under each other
    association (tests/test_w8a8_host.py counts them)."""
    c = C.gemm_inputs(dict(kind="exact", m=m, n=n, k=k, with_bias=with_bias))
    tile(t)
    v = C.gemm_bits(gemm_case(c), c)
    assert not v, v


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("t", TILES)
def test_gemm_saturation_needle(tile, t, with_bias):
    """K = 4304 with x = -128 (C.needle_case): sums beyond 2^24 and one that is not a float, landing on a tie of fp16."""
    c = C.needle_case(with_bias)
    tile(t)
    out = gemm_case(c)
    want = c["want"]
    assert torch.equal(bits(out), bits(want)), (out[:, ::8], want[:, ::8])


def _gemm_bounds(with_bias):
    """x and w inside larger buffers filled with 127, out inside a NaN buffer: a read past row M / N or column K would change the result, a
    write past the output would break the guard."""
    m, n, k = 65, 72, 208
    c = C.bounds_case(with_bias)
    x, w, ws, as_, bias = c["x"], c["w"], c["ws"], c["as_"], c["bias"]
    plain = gemm_case(c)
    pad = 4096
    xb = torch.full((pad + m * k + pad,), 127, dtype=torch.int8, device=DEV)
    wb = torch.full((pad + n * k + pad,), 127, dtype=torch.int8, device=DEV)
    ob = torch.full((pad + m * n + pad,), float("nan"), dtype=F16, device=DEV)
    xv, wv, ov = xb[pad:pad + m * k].view(m, k), wb[pad:pad + n * k].view(n, k), ob[pad:pad + m * n].view(m, n)
    xv.copy_(x)
    wv.copy_(w)
    if with_bias:
        _engine().w8a8_gemm_fuse_bias_forward_cuda(xv, wv, ws.to(DEV), as_.to(DEV), ov, bias.to(DEV))
    else:
        _engine().w8a8_gemm_forward_cuda(xv, wv, ws.to(DEV), as_.to(DEV), ov)
    torch.cuda.synchronize()
    assert torch.equal(bits(ov.cpu()), bits(plain)) and torch.equal(bits(plain), bits(c["want"]))
    assert torch.isnan(ob[:pad]).all() and torch.isnan(ob[pad + m * n:]).all()
    assert (xb[:pad] == 127).all() and (xb[pad + m * k:] == 127).all() and (wb[:pad] == 127).all() and (wb[pad + n * k:] == 127).all()


@pytest.mark.parametrize("t", TILES)
def test_gemm_bounds(tile, t):
    tile(t)
    _gemm_bounds(True)


@pytest.mark.parametrize("t", TILES)
def test_gemm_bounds_no_bias(tile, t):
    """The same guards around the instantiation without bias (w8a8_gemm_forward_cuda)."""
    tile(t)
    _gemm_bounds(False)


def check_gelu_stage(x, tmp, q, scale):
    v = C.check_gelu_stage(x, tmp, q, scale)
    assert not v, v


def gelu_both(x):
    E = _engine()
    k = x.shape[-1]
    res = []
    for f in (E.gelu_and_quant, lambda q, xx, s, t: ops.gelu_quant_per_token(xx, q, s, t)):
        q = torch.full(x.shape, 99, dtype=torch.int8, device=DEV)
        s = torch.full((x.numel() // k,), float("nan"), dtype=F16, device=DEV)
        tmp = torch.full(x.shape, float("nan"), dtype=F16, device=DEV)
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
    P = C.mlp_inputs()
    m, hid, ffn = P["m"], P["hid"], P["ffn"]
    w1, w2, ws1, ws2, b1, b2, h = [P[k].to(DEV) for k in ("w1", "w2", "ws1", "ws2", "b1", "b2", "h")]
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
        v = C.gemm_bound(o, dict(x=x8, w=w8, ws=ws, as_=as_, bias=b))
        assert not v, v

    within(fc1_, xq_, w1.cpu(), ws1, s0_, b1)
    v = C.check_gelu_stage(fc1_, tmp_, aq_, s1_)
    assert not v, v
    within(out_, aq_, w2.cpu(), ws2, s1_, b2)


def quant_both(x):
    """engine and ops -> (q, scale) on the CPU, equal bits."""
    E = _engine()
    k = x.shape[-1]
    xd = x.to(DEV)
    res = []
    for f in (E.invoke_quant, lambda q, xx, s: ops.quant_per_token(xx, q, s)):
        q = torch.full(x.shape, 99, dtype=torch.int8, device=DEV)
        s = torch.full((x.numel() // k,), float("nan"), dtype=F16, device=DEV)
        assert f(q, xd, s) is None
        res.append((q.cpu(), s.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(bits(res[0][1]), bits(res[1][1]))
    return res


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [16, 80, 1152, 4304])
@pytest.mark.parametrize("m", [1, 130])
def test_invoke_quant(dtype, m, k):
    x = C.quant_inputs(dtype, m, k)
    res = quant_both(x)
    qo, so = W.quant_per_token(x)
    for q, s in res:
        assert torch.equal(bits(s), bits(so)), (s[:4], so[:4])
        assert torch.equal(q, qo), int((q != qo).sum())
        assert C.quant_bits(q, s, x) == {}
    if m > 3:
        assert float(so[0]) == 0.0 and (qo[0] == 0).all() and int(qo[1].min()) == -127 and int(qo[1].max()) <= 0
        assert int(qo[2, 0]) == 127 and int(qo[2, k - 1]) == -127


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [16, 80])
def test_invoke_quant_needles(dtype, k):
    """Ties and infinities (C.quant_needle).  Rows 0-2: one +-127 makes the inverse exactly 1, every other element is a half-integer, so q is
    the nearest-even rounding of a tie: +-0.5 -> 0, +-1.5 and +-2.5 -> +-2, 125.5 -> 126, -126.5 -> -126.  Rows 3-4: one +-inf: scale inf,
    q all zero (finite * 0 = 0, inf * 0 = NaN -> 0).  The conversion is the one gelu_and_quant and rms_norm_general use as well."""
    x, q_want, s_want = C.quant_needle(dtype, k)
    for q, s in quant_both(x):
        assert torch.equal(q, q_want), (q[:, :9].tolist(), q_want[:, :9].tolist())
        assert torch.equal(bits(s), bits(s_want)), s
        assert C.quant_bits(q, s, x) == {}


def test_invoke_quant_refuses_float32():
    E = _engine()
    x = torch.zeros(2, 16, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        E.invoke_quant(torch.zeros(2, 16, dtype=torch.int8, device=DEV), x, torch.zeros(2, dtype=F16, device=DEV))
    with pytest.raises(TypeError, match="float16"):
        ops.quant_per_token(x, torch.zeros(2, 16, dtype=torch.int8, device=DEV), torch.zeros(2, dtype=F16, device=DEV))


@pytest.mark.parametrize("m,k", [(3, 80), (130, 4304)])
def test_gelu_and_quant_staged(m, k):
    x = C.gelu_inputs(m, k)  # rows 0 and 1 carry the quirk of the amax (positives up to 1e-4 do not count)
    tmp, q, s = gelu_both(x.to(DEV))
    check_gelu_stage(x, tmp, q, s)
    t = tmp.cpu().float()
    assert 0 < float(t[0].max()) <= 1e-4 and float(s[0]) == 0.0
    assert 0 < float(t[1].max()) <= 1e-4 and float(t[1].min()) < 0 and 0 < float(s[1]) * 127 < 0.5 * float(t[1].max())


def test_gelu_and_quant_overflow_rows():
    """+-1 500, +-30 000, +-65 504 among ordinary values (C.gelu_overflow_inputs): (0.044715h x) x overflows to inf in fp16, tanh saturates,
    positive x returns x and negative x returns -0.  The stage check is the unchanged one; on the planted values it is decided (the host
    test shows the candidates agree there), so those are compared bit for bit."""
    x, big = C.gelu_overflow_inputs()
    tmp, q, s = gelu_both(x.to(DEV))
    check_gelu_stage(x, tmp, q, s)
    t = tmp.cpu()
    pos, neg = big & (x > 0), big & (x < 0)
    assert torch.equal(bits(t)[pos], bits(x)[pos])
    assert (bits(t)[neg] == bits(torch.tensor(-0.0, dtype=F16))).all()
    assert torch.isfinite(t.float()).all() and torch.isfinite(s.cpu().float()).all()
    assert [int(v) for v in q.cpu().abs().amax(-1)] == [127] * x.shape[0]


def ln_both(c):
    """engine and ops -> (q, scaling) on the CPU, equal bits."""
    E = _engine()
    x, gamma, beta = c["x"].to(DEV), c["gamma"].to(DEV), _dev(c["beta"])
    res = []
    for via_ops in (False, True):
        q = torch.full(x.shape, 99, dtype=torch.int8, device=DEV)
        s = c["scaling"].to(DEV).clone()
        if via_ops:
            ops.layernorm_quant(x, gamma, beta, s, q, c["eps"], c["per_token"])
        else:
            assert E.rms_norm_general(q, x, gamma, beta, s, c["eps"], c["per_token"]) is None
        res.append((q.cpu(), s.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(bits(res[0][1]), bits(res[1][1]))
    return res[0]


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [80, 1152, 4304])
@pytest.mark.parametrize("mode", ["token", "token_no_beta", "tensor"])
def test_rms_norm_general(dtype, k, mode):
    """|q - y64| <= 0.5 + 127 * 2^-10 + s and |scale - amax64 / 127| <= 0.5 ulp_fp16 + 2^-10 amax64 / 127, y64 = the float64 value with
    amax over T-rounded v; s is the fp32 evaluation slack (C.ln_bound derives it).  Per token the peak of q is 127; per tensor scaling is
    only read.  token_no_beta: beta = None (the C entry's NULL, the binding's bias=None)."""
    E = _engine()
    c = C.ln_inputs(dtype, k, mode)
    x, gamma, beta, scaling = c["x"], c["gamma"], c["beta"], c["scaling"]
    q, s = ln_both(c)
    v = C.ln_bound(q, s, c)
    assert not v, v
    if mode == "tensor":
        nobeta = torch.full(x.shape, 99, dtype=torch.int8, device=DEV)
        E.rms_norm_general(nobeta, x.to(DEV), gamma.to(DEV), torch.zeros_like(beta).to(DEV), scaling.to(DEV), c["eps"], False)
        assert torch.equal(nobeta.cpu(), q)  # beta is ignored in this mode (layernorm.cu:224-229)


@pytest.mark.parametrize("check", [c for c in C.LN_CHECKS if c["kind"] in ("eps_small", "eps_big")], ids=lambda c: c["id"])
def test_rms_norm_general_eps(check):
    """Inputs on which eps counts, under the unchanged bound (its derivation needs |mean| <= std, asserted per row, and a larger var + eps
    only shrinks the error): the rows' std scaled by 1e-3 with eps = 1e-6 (var 2.5e-7 .. 6e-6), and the unscaled rows with eps = 1e-2.
    A kernel that drops eps, or adds it outside the root, fails these (tests/test_w8a8_host.py) and none of test_rms_norm_general."""
    c = C.ln_check_inputs(check)
    q, s = ln_both(c)
    v = C.ln_bound(q, s, c)
    assert not v, v


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
def test_rms_norm_general_per_tensor_reads_element_zero(dtype):
    """scaling = [25, 3, 4, 5, ..]: q follows element 0 and the tensor comes back unchanged; a one-element scaling gives the same q."""
    c = C.ln_check_inputs(dict(kind="scaling", dtype=dtype, k=80, mode="tensor"))
    assert c["scaling"][:4].tolist() == [25.0, 3.0, 4.0, 5.0]
    q, s = ln_both(c)
    v = C.ln_bound(q, s, c)
    assert not v, v
    q1, s1 = ln_both(dict(c, scaling=c["scaling"][:1].clone()))
    assert torch.equal(q1, q) and s1.tolist() == [25.0]


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [8, 2048, 2056, 16376, 16384])
def test_rms_norm_general_register_depth(dtype, k):
    """One to eight register vectors per thread: a thread holds vector t of the row at column 8 (thread + 256 t), so K = 2048 fills the
    first vector of every thread, 2056 starts the second, 16384 fills all eight.  The bound is C.ln_bound with the depth of the fp32 sums
    re-derived for K = 16384: a thread adds 8 vectors x 8 elements = 64 terms, the wave reduces in 6 shuffle steps, and the four waves'
    sums take 3 more additions: 73 (the 72 of the shorter rows was an upper bound for their 3 x 8 + 6 + 3 = 33)."""
    assert C.DEPTH_16384 == 8 * 8 + 6 + 3
    c = C.ln_check_inputs(dict(kind="depth", dtype=dtype, k=k, mode="token"))
    assert c["depth"] == C.DEPTH_16384 and c["x"].shape == (3, k)
    q, s = ln_both(c)
    v = C.ln_bound(q, s, c)
    assert not v, v


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
def test_rms_norm_general_refuses_rows_longer_than_16384(dtype):
    E = _engine()
    m, k = 2, C.LN_MAX_K + 8
    x, g = torch.zeros(m, k, dtype=dtype, device=DEV), torch.ones(k, dtype=dtype, device=DEV)
    q, s = torch.full((m, k), 99, dtype=torch.int8, device=DEV), torch.full((m,), 7.0, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="16384"):
        E.rms_norm_general(q, x, g, g, s, 1e-6, True)
    with pytest.raises(_capi.AwqNativeError):
        ops.layernorm_quant(x, g, g, s, q, 1e-6, True)
    torch.cuda.synchronize()
    assert (q == 99).all() and (s == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------------
# leading dimensions and views
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
@pytest.mark.parametrize("k", [16, 80])
def test_leading_dimensions_give_the_bits_of_the_flat_rows(dtype, k):
    """[2, 19, K] inputs and outputs against the same data as [38, K], for the three quantisers."""
    x = C.quant_inputs(dtype, 38, k)
    (q2, s2), _ = quant_both(x)
    (q3, s3), _ = quant_both(x.reshape(2, 19, k))
    assert q3.shape == (2, 19, k) and torch.equal(q3.reshape(38, k), q2) and torch.equal(bits(s3), bits(s2))
    assert C.quant_bits(q3, s3, x.reshape(2, 19, k)) == {}
    if k == 80:  # (at K = 16 the sample mean of a row can exceed its std, which the bound's derivation excludes)
        c = C.ln_inputs(dtype, k, "token", m=38)
        q2, s2 = ln_both(c)
        c3 = dict(c, x=c["x"].reshape(2, 19, k))
        q3, s3 = ln_both(c3)
        assert q3.shape == (2, 19, k) and torch.equal(q3.reshape(38, k), q2) and torch.equal(bits(s3), bits(s2))
        v = C.ln_bound(q3, s3, c3)
        assert not v, v
    if dtype == F16:
        x = C.gelu_inputs(38, k)
        t2, q2, s2 = [t.cpu() for t in gelu_both(x.to(DEV))]
        t3, q3, s3 = [t.cpu() for t in gelu_both(x.reshape(2, 19, k).to(DEV))]
        assert t3.shape == (2, 19, k) and torch.equal(bits(t3.reshape(38, k)), bits(t2)) and torch.equal(q3.reshape(38, k), q2)
        assert torch.equal(bits(s3), bits(s2))
        check_gelu_stage(x.reshape(2, 19, k), t3, q3, s3)


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16])
def test_non_contiguous_inputs_are_refused_before_any_launch(dtype):
    """A column slice of a wider buffer: refused by the binding ("contiguous tensors on one GPU") and by ops; the outputs stay untouched."""
    E = _engine()
    m, k = 38, 80
    wide = torch.ones(m, 2 * k, dtype=dtype, device=DEV)
    x = wide[:, :k]
    assert not x.is_contiguous()
    g = torch.ones(k, dtype=dtype, device=DEV)
    q = torch.full((m, k), 99, dtype=torch.int8, device=DEV)
    s = torch.full((m,), 7.0, dtype=F16, device=DEV)
    tmp = torch.full((m, k), 5.0, dtype=F16, device=DEV)
    msg = "contiguous tensors on one GPU"
    with pytest.raises(RuntimeError, match=msg):
        E.invoke_quant(q, x, s)
    with pytest.raises(RuntimeError, match=msg):
        E.rms_norm_general(q, x, g, g, s, 1e-6, True)
    with pytest.raises(ValueError, match="contiguous"):
        ops.quant_per_token(x, q, s)
    with pytest.raises(ValueError, match="contiguous"):
        ops.layernorm_quant(x, g, g, s, q, 1e-6, True)
    if dtype == F16:
        with pytest.raises(RuntimeError, match=msg):
            E.gelu_and_quant(q, x, s, tmp)
        with pytest.raises(ValueError, match="contiguous"):
            ops.gelu_quant_per_token(x, q, s, tmp)
        with pytest.raises(RuntimeError, match=msg):  # a non-contiguous output is refused as well
            E.gelu_and_quant(q, x.contiguous(), s, wide[:, k:])
    torch.cuda.synchronize()
    assert (q == 99).all() and (s == 7.0).all() and (tmp == 5.0).all() and (wide == 1).all()


# ------------------------------------------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------------------------------------------
def _linear(n, k, bias, seed):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        lin.weight.mul_(3.0)
    return lin.half()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", ["linear", "qkv"])
def test_module_forward_writes_the_bits_of_the_direct_call(kind, with_bias):
    """W8A8OF16LinearDynamicInputScale.from_linear / .from_qkv: the buffers are W.quantize_weight of the source weights (q, k, v
    concatenated in that order), bias is a plain attribute on the GPU that the state dict does not carry, forward(x_q, scale, out) writes
    what the engine writes with those buffers -- which is the specified epilogue, bit for bit -- and an init_only module that loads the
    state dict and is handed the bias reproduces it."""
    E = _engine()
    m, k, n = 65, 80, 48
    if kind == "linear":
        lins = [_linear(n, k, with_bias, 1)]
        mod = W8A8OF16LinearDynamicInputScale.from_linear(lins[0])
        blank = W8A8OF16LinearDynamicInputScale.from_linear(lins[0], init_only=True)
    else:
        lins = [_linear(n, k, with_bias, 2 + i) for i in range(3)]
        mod = W8A8OF16LinearDynamicInputScale.from_qkv(*lins)
        blank = W8A8OF16LinearDynamicInputScale.from_qkv(*lins, init_only=True)
    weight = torch.cat([l.weight.data for l in lins], 0)
    N = weight.shape[0]
    qo, so = W.quantize_weight(weight)
    assert mod.weight.is_cuda and mod.dequant_scale.is_cuda and (mod.in_features, mod.out_features) == (k, N)
    assert torch.equal(mod.weight.cpu(), qo) and torch.equal(bits(mod.dequant_scale.cpu()), bits(so))
    assert set(mod.state_dict().keys()) == {"weight", "dequant_scale"}
    if with_bias:
        assert mod.bias.is_cuda and mod.bias.dtype == F16 and not isinstance(mod.bias, torch.nn.Parameter)
        assert torch.equal(mod.bias.cpu(), torch.cat([l.bias.data for l in lins]).half())
    else:
        assert mod.bias is None
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(65)) * 2).to(F16)
    xq, sc = W.quant_per_token(x)
    xq_d, sc_d = xq.to(DEV), sc.to(DEV)
    out = torch.full((m, N), float("nan"), dtype=F16, device=DEV)
    assert mod(xq_d, sc_d, out) is None
    direct = torch.full((m, N), float("nan"), dtype=F16, device=DEV)
    if with_bias:
        E.w8a8_gemm_fuse_bias_forward_cuda(xq_d, mod.weight, mod.dequant_scale, sc_d, direct, mod.bias)
    else:
        E.w8a8_gemm_forward_cuda(xq_d, mod.weight, mod.dequant_scale, sc_d, direct)
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(direct.cpu()))
    c = dict(x=xq, w=qo, ws=so, as_=sc, bias=mod.bias.cpu() if with_bias else None)
    v = C.gemm_bits(out.cpu(), dict(c, want=C.gemm_stand_in(c)))
    assert not v, v
    blank = blank.to(DEV)
    blank.load_state_dict(mod.state_dict())
    assert (blank.bias is None) == (not with_bias)
    if with_bias:
        blank.bias = mod.bias
    again = torch.full((m, N), float("nan"), dtype=F16, device=DEV)
    blank(xq_d, sc_d, again)
    torch.cuda.synchronize()
    assert torch.equal(bits(again.cpu()), bits(out.cpu()))


# ------------------------------------------------------------------------------------------------------------------------
# the attention half of a tower layer
# ------------------------------------------------------------------------------------------------------------------------
def test_attention_half_of_a_tower_layer_staged():
    """rms_norm_general (per token) -> qkv GEMM with bias -> split / reshape (views) -> flash_attn_func(causal=False) -> invoke_quant into
    the SAME int8 and scale buffers -> out_proj GEMM with bias: the counterpart of the fc1 -> GELU -> fc2 test.  E = 256, 4 heads of 64
    (SigLIP's head dim 72 is not served by the attention kernel), 2 x 70 tokens, fp16.  Every stage is checked against its oracle fed with
    the GPU's previous stage: the layernorm bound, gemm_f32 bits, the prefill attention bound, quant_per_token bits, gemm_f32 bits.  The
    sequence runs twice through the engine and once through llm_awq_amd.ops: equal bits."""
    E = _engine()
    flash = _flash()
    L = C.layer_inputs()
    bsz, seqlen, heads, dh, emb, m, ln = [L[k] for k in ("bsz", "seqlen", "heads", "dh", "emb", "m", "ln")]
    d = {k: v.to(DEV) for k, v in dict(h=ln["x"], gamma=ln["gamma"], beta=ln["beta"], wqkv=L["wqkv"], wo=L["wo"], ws_qkv=L["ws_qkv"],
                                       ws_o=L["ws_o"], b_qkv=L["b_qkv"], b_o=L["b_o"]).items()}
    xq = torch.empty(m, emb, dtype=torch.int8, device=DEV)
    scale = torch.empty(m, dtype=F16, device=DEV)
    qkv = torch.empty(m, 3 * emb, dtype=F16, device=DEV)
    out = torch.empty(m, emb, dtype=F16, device=DEV)

    def run(via_ops):
        if via_ops:
            ops.layernorm_quant(d["h"], d["gamma"], d["beta"], scale, xq, ln["eps"], True)
        else:
            E.rms_norm_general(xq, d["h"], d["gamma"], d["beta"], scale, ln["eps"], True)
        x0, s0 = xq.clone(), scale.clone()
        if via_ops:
            ops.w8a8_gemm(xq, d["wqkv"], d["ws_qkv"], scale, qkv, d["b_qkv"])
        else:
            E.w8a8_gemm_fuse_bias_forward_cuda(xq, d["wqkv"], d["ws_qkv"], scale, qkv, d["b_qkv"])
        q, k, v = [t.reshape(bsz, seqlen, heads, dh) for t in qkv.split(emb, dim=-1)]
        assert q.data_ptr() == qkv.data_ptr() and v.data_ptr() == qkv.data_ptr() + 4 * emb and q.stride() == (seqlen * 3 * emb, 3 * emb, dh, 1)
        attn = (ops.flash_attn_func(q, k, v, None, False) if via_ops else flash(q, k, v, causal=False)).reshape(m, emb)
        if via_ops:
            ops.quant_per_token(attn, xq, scale)
            ops.w8a8_gemm(xq, d["wo"], d["ws_o"], scale, out, d["b_o"])
        else:
            E.invoke_quant(xq, attn, scale)
            E.w8a8_gemm_fuse_bias_forward_cuda(xq, d["wo"], d["ws_o"], scale, out, d["b_o"])
        return [t.clone() for t in (x0, s0, qkv, attn, xq, scale, out)]

    first, second, third = run(False), run(False), run(True)
    torch.cuda.synchronize()
    for other in (second, third):
        for a, b in zip(first, other):
            assert torch.equal(bits(a), bits(b))

    x0, s0, qkv_, attn_, x1, s1, out_ = [t.cpu() for t in first]
    v = C.ln_bound(x0, s0, ln)
    assert not v, v
    v = C.gemm_stage(qkv_, x0, L["wqkv"], L["ws_qkv"], s0, L["b_qkv"])
    assert not v, v
    v = C.attention_stage(attn_, qkv_, L)
    assert not v, v
    v = C.quant_bits(x1, s1, attn_)
    assert not v, v
    v = C.gemm_stage(out_, x1, L["wo"], L["ws_o"], s1, L["b_o"])
    assert not v, v
