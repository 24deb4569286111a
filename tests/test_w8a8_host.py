"""The W8A8 family without a GPU: the C entries' argument codes, the GEMM's plan, the weight quantiser of llm_awq_amd.w8a8_linear against
its restatement (tests/w8a8_oracle.py), the modules' state-dict keys and the engine's five exports."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.w8a8_linear import W8A8OF16LinearDynamicInputScale, W8A8OF16LinearStaticScale, quantize_weight_per_channel
from tests import w8a8_oracle as W

OK, ERR_DTYPE, ERR_SHAPE, ERR_ALIGN, ERR_NULL = 0, -3, -4, -5, -6
P, ODD = 0x10000, 0x10008  # a 16-byte aligned and a misaligned fake device address: every call below is refused before any GPU call

SIGLIP = [(3456, 1152), (1152, 1152), (4304, 1152), (1152, 4304)]    # SigLIP-so400m (N, K): qkv, out, fc1, fc2
INTERNVIT = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]  # InternViT-300M
ROWS = [1, 128, 129, 729, 5832]


def test_gemm_argument_codes():
    L = _capi.lib()
    g = L.awq_w8a8_gemm
    assert g(None, P, P, P, None, P, 4, 16, 16, None) == ERR_NULL
    assert g(P, None, P, P, None, P, 4, 16, 16, None) == ERR_NULL
    assert g(P, P, None, P, None, P, 4, 16, 16, None) == ERR_NULL
    assert g(P, P, P, None, None, P, 4, 16, 16, None) == ERR_NULL
    assert g(P, P, P, P, None, None, 4, 16, 16, None) == ERR_NULL
    assert g(P, P, P, P, None, P, 4, 16, 24, None) == ERR_SHAPE   # k % 16
    assert g(P, P, P, P, None, P, 4, 12, 16, None) == ERR_SHAPE   # n % 8
    assert g(P, P, P, P, None, P, 0, 16, 16, None) == ERR_SHAPE   # m < 1
    assert g(P, P, P, P, None, P, 4, 16, 0, None) == ERR_SHAPE
    for bad in range(6):
        a = [P, P, P, P, P, P]
        a[bad] = ODD
        assert g(a[0], a[1], a[2], a[3], a[4], a[5], 4, 16, 16, None) == ERR_ALIGN, bad


def test_quantiser_argument_codes():
    L = _capi.lib()
    q = L.awq_quant_per_token
    assert q(None, P, P, 2, 16, 0, None) == ERR_NULL and q(P, None, P, 2, 16, 0, None) == ERR_NULL and q(P, P, None, 2, 16, 0, None) == ERR_NULL
    assert q(P, P, P, 2, 16, 2, None) == ERR_DTYPE
    assert q(P, P, P, 2, 12, 0, None) == ERR_SHAPE and q(P, P, P, 0, 16, 1, None) == ERR_SHAPE
    assert q(ODD, P, P, 2, 16, 0, None) == ERR_ALIGN and q(P, ODD, P, 2, 16, 0, None) == ERR_ALIGN and q(P, P, ODD, 2, 16, 1, None) == ERR_ALIGN
    g = L.awq_gelu_quant_per_token
    for i in range(4):
        a = [P, P, P, P]
        a[i] = None
        assert g(*a, 2, 16, None) == ERR_NULL
        a[i] = ODD
        assert g(*a, 2, 16, None) == ERR_ALIGN
    assert g(P, P, P, P, 2, 20, None) == ERR_SHAPE and g(P, P, P, P, 0, 16, None) == ERR_SHAPE
    n = L.awq_layernorm_quant
    assert n(None, P, P, 1e-6, P, P, 2, 16, 1, 0, None) == ERR_NULL and n(P, None, P, 1e-6, P, P, 2, 16, 1, 0, None) == ERR_NULL
    assert n(P, P, None, 1e-6, None, P, 2, 16, 1, 0, None) == ERR_NULL and n(P, P, None, 1e-6, P, None, 2, 16, 1, 0, None) == ERR_NULL
    assert n(P, P, P, 1e-6, P, P, 2, 16, 1, 7, None) == ERR_DTYPE
    assert n(P, P, P, 1e-6, P, P, 2, 12, 1, 0, None) == ERR_SHAPE and n(P, P, P, 1e-6, P, P, 2, 16392, 0, 1, None) == ERR_SHAPE  # k <= 16384
    assert n(P, P, ODD, 1e-6, P, P, 2, 16, 1, 0, None) == ERR_ALIGN and n(P, P, None, 1e-6, ODD, P, 2, 16, 0, 1, None) == ERR_ALIGN


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("n,k", SIGLIP + INTERNVIT)
def test_gemm_plan_is_pinned_for_the_towers(m, n, k):
    """One rule: the 128 x 128 tile when it yields at least 256 blocks (one per CU), else 64 x 64.  Of the towers' shapes only the 5832-row
    batch (46 row tiles x >= 8 column tiles) reaches that; 729 rows give at most 6 x 34 = 204 tiles of 128."""
    blocks, tm, tn = ops.w8a8_gemm_plan(m, n, k)
    want = 128 if m == 5832 else 64
    assert (tm, tn) == (want, want)
    assert blocks == -(-m // tm) * -(-n // tn)


def test_gemm_plan_rule_boundary_and_unserved_shapes():
    assert ops.w8a8_gemm_plan(2048, 2048, 64) == (256, 128, 128)          # 16 x 16 tiles of 128: exactly one per CU
    assert ops.w8a8_gemm_plan(2048, 1920, 64) == (32 * 30, 64, 64)        # 16 x 15 = 240 < 256
    assert ops.w8a8_gemm_plan(1, 8, 16) == (1, 64, 64)
    L = _capi.lib()
    assert L.awq_w8a8_gemm_plan(4, 16, 16, None, None) == 1                # the tile pointers are optional
    for m, n, k in [(4, 16, 24), (4, 16, 8), (4, 12, 16), (4, 4, 16), (0, 16, 16), (4, 16, 0)]:
        assert ops.w8a8_gemm_plan(m, n, k)[0] == 0, (m, n, k)


def _linear(n, k, dtype, bias=True, zero_row=None):
    lin = torch.nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        lin.weight.mul_(3.0)
        if zero_row is not None:
            lin.weight[zero_row].zero_()
    return lin.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_weight_quantiser_matches_its_restatement(dtype):
    lin = _linear(24, 80, dtype, zero_row=5)
    w0 = lin.weight.data.clone()
    q, s = quantize_weight_per_channel(lin.weight.data)
    assert torch.equal(lin.weight.data, w0)  # (the reference divides the caller's weight in place; this does not)
    qo, so = W.quantize_weight(w0)
    assert q.dtype == torch.int8 and s.dtype == dtype and s.shape == (24, 1)
    assert torch.equal(q.cpu(), qo)
    assert torch.equal(s.reshape(-1).half().cpu().view(torch.int16), so.view(torch.int16))
    assert (q[5] == 0).all() and float(s[5]) > 0  # the clamp: a row of zeros gets the floor scale, not a division by zero
    assert int(q.abs().max()) == 127

    m = W8A8OF16LinearDynamicInputScale.from_linear(lin)
    assert torch.equal(m.weight.cpu(), qo) and torch.equal(m.dequant_scale.cpu().view(torch.int16), so.view(torch.int16))
    assert m.weight.dtype == torch.int8 and m.dequant_scale.dtype == torch.float16 and m.bias.dtype == torch.float16
    assert torch.equal(m.bias.cpu(), lin.bias.data.half())
    assert m.bias.device == m.weight.device


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_from_qkv_quantises_the_concatenation(dtype):
    q, k, v = _linear(16, 48, dtype), _linear(8, 48, dtype), _linear(8, 48, dtype, zero_row=0)
    m = W8A8OF16LinearDynamicInputScale.from_qkv(q, k, v)
    cat = torch.cat([q.weight.data, k.weight.data, v.weight.data], 0)
    qo, so = W.quantize_weight(cat)
    assert m.in_features == 48 and m.out_features == 32
    assert torch.equal(m.weight.cpu(), qo) and torch.equal(m.dequant_scale.cpu().view(torch.int16), so.view(torch.int16))
    assert torch.equal(m.bias.cpu(), torch.cat([q.bias.data, k.bias.data, v.bias.data]).half())
    nb = W8A8OF16LinearDynamicInputScale.from_qkv(*[_linear(8, 16, dtype, bias=False) for _ in range(3)])
    assert nb.bias is None


def test_state_dict_keys_and_init_only():
    for cls in (W8A8OF16LinearStaticScale, W8A8OF16LinearDynamicInputScale):
        for bias in (True, False):
            m = cls(32, 16, bias)
            assert set(m.state_dict().keys()) == {"weight", "dequant_scale"}  # bias is a plain attribute in the reference: not a key
            assert m.weight.shape == (16, 32) and m.weight.dtype == torch.int8
            assert m.dequant_scale.shape == (16,) and m.dequant_scale.dtype == torch.float16
            assert (m.bias is None) == (not bias)
    m = W8A8OF16LinearDynamicInputScale.from_linear(torch.nn.Linear(32, 16), init_only=True)
    sd = {"weight": torch.ones(16, 32, dtype=torch.int8), "dequant_scale": torch.full((16,), 0.5, dtype=torch.float16)}
    m.load_state_dict(sd)
    assert torch.equal(m.weight.cpu(), sd["weight"])
    with pytest.raises(NotImplementedError):
        W8A8OF16LinearStaticScale(32, 16)(torch.zeros(1, 32, dtype=torch.int8))


def test_engine_exposes_the_five_names_and_refuses_cpu_and_float32():
    eng = llm_awq_amd.load_engine()
    for name in ("w8a8_gemm_forward_cuda", "w8a8_gemm_fuse_bias_forward_cuda", "invoke_quant", "gelu_and_quant", "rms_norm_general"):
        assert callable(getattr(eng, name)), name
    x = torch.zeros(2, 16, dtype=torch.float16)
    q = torch.zeros(2, 16, dtype=torch.int8)
    s = torch.zeros(2, dtype=torch.float16)
    g = torch.ones(16, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.invoke_quant(q, x, s)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.gelu_and_quant(q, x, s, x.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        eng.rms_norm_general(q, x, g, g, s, 1e-6)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.w8a8_gemm_forward_cuda(q, q.clone(), s, s, torch.zeros(2, 2, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float32"):
        eng.invoke_quant(q, x.float(), s)
    with pytest.raises(RuntimeError, match="float32"):
        eng.gelu_and_quant(q, x.float(), s, x.clone())
    with pytest.raises(RuntimeError, match="float32"):
        eng.rms_norm_general(out=q, input=x.float(), weight=g, bias=g, scaling=s, epsilon=1e-6, use_per_token_quant=False)
    with pytest.raises(RuntimeError, match="float32"):
        eng.w8a8_gemm_fuse_bias_forward_cuda(q, q.clone(), s, s, torch.zeros(2, 2), s)
    with pytest.raises(_capi.AwqNativeError):
        ops.quant_per_token(x, q, s)


def test_oracle_self_checks():
    """The restatements agree with plain formulas where those are unambiguous."""
    x = torch.tensor([[1.0, -2.0, 0.5, 0.25] * 4, [0.0] * 16], dtype=torch.float16)
    q, s = W.quant_per_token(x)
    assert q[0, :4].tolist() == [64, -127, 32, 16] and (q[1] == 0).all() and float(s[1]) == 0.0   # 63.5 and 31.75 -> nearest even / nearest
    assert float(s[0]) == float(torch.tensor(2.0 / 127.0).half())
    assert W.sat_s8(torch.tensor([float("nan"), float("inf"), -1e9, 0.5, 1.5, 2.5])).tolist() == [0, 127, -128, 0, 2, 2]
    lo, hi = W.gelu_candidates(torch.tensor([[0.0, 1.0, -1.0, 3.0]], dtype=torch.float16), 2.0 ** -22)
    ref = torch.nn.functional.gelu(torch.tensor([0.0, 1.0, -1.0, 3.0]), approximate="tanh")
    assert float((lo.float()[0] - ref).abs().max()) < 2e-3 and float((hi.float()[0] - ref).abs().max()) < 2e-3
    g = torch.tensor([[0.00009, -0.5, 0.25, 0.0] * 2, [0.00009, 0.00005, 0.0, 0.0] * 2], dtype=torch.float16)
    qg, sg = W.gelu_quant_from_tmp(g)
    assert float(sg[0]) == float(torch.tensor(0.5 / 127.0).half())
    assert float(sg[1]) == 0.0 and qg[1].tolist() == [127, 127, 0, 0] * 2  # only tiny positives: amax stays 0, 127 / 0 = inf, inf * g saturates
    acc = W.acc_exact(torch.full((1, 4304), -128, dtype=torch.int8), torch.full((1, 4304), -128, dtype=torch.int8))
    assert int(acc) == 70516736
