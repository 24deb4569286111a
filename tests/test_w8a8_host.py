"""The W8A8 family without a GPU: the C entries' argument codes, the GEMM's plan, the weight quantiser of llm_awq_amd.w8a8_linear against
its restatement (tests/w8a8_oracle.py), the modules' state-dict keys and the engine's five exports -- and the proof that the checks of
tests/test_gpu_w8a8.py are sound and sharp: every criterion of tests/w8a8_cases.py passes the restatement in the kernel's place and
rejects it with any one applicable fault switched in."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.w8a8_linear import W8A8OF16LinearDynamicInputScale, W8A8OF16LinearStaticScale, quantize_weight_per_channel
from tests import w8a8_cases as C
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


# ------------------------------------------------------------------------------------------------------------------------
# the GPU checks are sound (the restatement passes) and sharp (the restatement with one fault does not)
# ------------------------------------------------------------------------------------------------------------------------
def _id(check):
    return check["id"]


def test_check_lists_cover_the_axes():
    for checks in (C.GEMM_CHECKS, C.QUANT_CHECKS, C.GELU_CHECKS, C.LN_CHECKS):
        assert len({c["id"] for c in checks}) == len(checks)
    g = {(c["kind"], c["with_bias"]) for c in C.GEMM_CHECKS}
    assert g == {(k, b) for k in ("lattice", "random", "exact", "needle", "bounds") for b in (False, True)}
    assert {(c["m"], c["n"], c["k"]) for c in C.GEMM_CHECKS if c["kind"] == "exact"} == {(300, 1152, 4304), (65, 272, 208)}
    assert {(c["dtype"], c["k"]) for c in C.QUANT_CHECKS if c["kind"] == "needle"} == {(d, k) for d in (C.F16, C.BF16) for k in (16, 80)}
    ln = {(c["kind"], c["dtype"], c["k"], c["mode"]) for c in C.LN_CHECKS}
    for d in (C.F16, C.BF16):
        for k in (80, 1152):
            assert {("eps_small", d, k, "token"), ("eps_small", d, k, "tensor"), ("eps_big", d, k, "token")} <= ln
        for k in (8, 2048, 2056, 16376, 16384):
            assert ("depth", d, k, "token") in ln
    # K = 2048 fills one register vector per thread exactly, 2056 starts the second, 16384 fills all eight
    assert 2048 == 256 * 8 and C.LN_MAX_K == 256 * 8 * 8


@pytest.mark.parametrize("check", C.GEMM_CHECKS, ids=_id)
def test_gemm_check_passes_the_oracle_and_sees_faults(check):
    c, crit = C.gemm_inputs(check), C.gemm_criterion(check)
    assert crit(C.gemm_stand_in(c), c) == {}
    for mutant in W.GEMM_MUTANTS:
        if C.gemm_mutant_applies(check, mutant):
            assert crit(C.gemm_stand_in(c, mutant), c) != {}, mutant


def test_epilogue_associations_differ_in_the_large_bit_exact_case():
    """Each wrong association of the epilogue changes at least 4 fp16 results of the (300, 1152, 4304) case: the bit-exact GPU check has
    something to see.  (The counts with this seed: assoc 11, nofma 8, assoc_bias 17, exact 17.)"""
    for with_bias, mutants in ((False, ("assoc",)), (True, ("nofma", "assoc_bias", "exact"))):
        c = C.gemm_inputs(dict(kind="exact", m=300, n=1152, k=4304, with_bias=with_bias))
        for mutant in mutants:
            n = C.gemm_bits(C.gemm_stand_in(c, mutant), c).get("bits", 0)
            print(mutant, n)
            assert n >= 4, (mutant, n)


@pytest.mark.parametrize("check", C.QUANT_CHECKS, ids=_id)
def test_quant_check_passes_the_oracle_and_sees_faults(check):
    x = C.quant_check_inputs(check)
    assert C.quant_bits(*C.quant_stand_in(x), x) == {}
    for mutant in W.QUANT_MUTANTS:
        if C.quant_mutant_applies(check, mutant):
            assert C.quant_bits(*C.quant_stand_in(x, mutant), x) != {}, mutant


@pytest.mark.parametrize("dtype", [C.F16, C.BF16])
@pytest.mark.parametrize("k", [16, 80])
def test_quant_needle_values_are_what_the_restatement_gives(dtype, k):
    x, q, s = C.quant_needle(dtype, k)
    qo, so = W.quant_per_token(x)
    assert torch.equal(qo, q) and torch.equal(C.bits(so), C.bits(s))
    assert qo[0, :9].tolist() == [127, 0, 2, -2, 2, -2, 126, -126, 4] and (qo[3:] == 0).all() and torch.isinf(so[3:]).all()
    away, _ = W.quant_per_token(x, "half_away")
    assert away[0, :9].tolist() == [127, -1, 2, -2, 3, -3, 126, -127, 4]  # what a round-half-away conversion would return


@pytest.mark.parametrize("check", C.GELU_CHECKS, ids=_id)
def test_gelu_check_passes_the_oracle_and_sees_faults(check):
    x = C.gelu_check_inputs(check)
    for hi in (False, True):  # either candidate is accepted
        assert C.check_gelu_stage(x, *C.gelu_stand_in(x, None, hi)) == {}
    for mutant in W.GELU_MUTANTS:
        if C.gelu_mutant_applies(check, mutant):
            assert C.check_gelu_stage(x, *C.gelu_stand_in(x, mutant)) != {}, mutant


def test_gelu_overflow_rows_are_decided():
    """On the planted values the candidates agree (tanh is exactly +-1): g = x for positive x, -0 for negative x."""
    x, big = C.gelu_overflow_inputs()
    lo, hi = W.gelu_candidates(x, C.TANH_DELTA)
    assert torch.equal(C.bits(lo)[big], C.bits(hi)[big])
    pos, neg = big & (x > 0), big & (x < 0)
    assert pos.any() and neg.any() and torch.equal(C.bits(lo)[pos], C.bits(x)[pos])
    assert (C.bits(lo)[neg] == C.bits(torch.tensor(-0.0, dtype=C.F16))).all()
    u, _ = W.gelu_fast_steps(x)
    assert torch.isinf(u[big]).all() and torch.isfinite(u[~big]).all()
    assert torch.isfinite(lo.float()).all()


@pytest.mark.parametrize("check", C.LN_CHECKS, ids=_id)
def test_layernorm_check_passes_the_oracle_and_sees_faults(check):
    c = C.ln_check_inputs(check)
    assert C.ln_bound(*C.ln_stand_in(c), c) == {}
    for mutant in W.LN_MUTANTS:
        if C.ln_mutant_applies(check, mutant):
            assert C.ln_bound(*C.ln_stand_in(c, mutant), c) != {}, mutant


def test_every_fault_is_seen_by_some_case():
    for mutants, checks, applies in ((W.GEMM_MUTANTS, C.GEMM_CHECKS, C.gemm_mutant_applies), (W.QUANT_MUTANTS, C.QUANT_CHECKS, C.quant_mutant_applies),
                                     (W.GELU_MUTANTS, C.GELU_CHECKS, C.gelu_mutant_applies), (W.LN_MUTANTS, C.LN_CHECKS, C.ln_mutant_applies)):
        seen = {m: sum(applies(c, m) for c in checks) for m in mutants}
        assert all(v > 0 for v in seen.values()), seen
    with pytest.raises(ValueError):
        W.gemm_f32(torch.zeros(1, 1, dtype=torch.int64), torch.ones(1), torch.ones(1), None, mutant="no such fault")


def _mlp_chain(gemm=None, quant=None, gelu=None):
    """The fc1 -> GELU -> fc2 sequence with the restatements as the kernels; -> the violations of the GPU test's four stage checks."""
    P = C.mlp_inputs()
    xq, s0 = C.quant_stand_in(P["h"], quant)
    c1 = dict(x=xq, w=P["w1"], ws=P["ws1"], as_=s0, bias=P["b1"])
    fc1 = C.gemm_stand_in(c1, gemm)
    tmp, aq, s1 = C.gelu_stand_in(fc1, gelu)
    c2 = dict(x=aq, w=P["w2"], ws=P["ws2"], as_=s1, bias=P["b2"])
    out = C.gemm_stand_in(c2, gemm)
    return [C.quant_bits(xq, s0, P["h"]), C.gemm_bound(fc1, c1), C.check_gelu_stage(fc1, tmp, aq, s1), C.gemm_bound(out, c2)]


def test_mlp_sequence_checks_pass_the_oracle_and_see_faults():
    assert _mlp_chain() == [{}, {}, {}, {}]
    for mutant in ("trunc", "inv_from_scale"):
        assert _mlp_chain(quant=mutant)[0] != {}, mutant
    for mutant in ("bias_first", "droptail"):  # (fc2 has K = 4304, K % 64 = 16)
        assert _mlp_chain(gemm=mutant)[3] != {}, mutant
    for mutant in ("single_rounding", "prod_f32", "inv_f32"):
        assert _mlp_chain(gelu=mutant)[2] != {}, mutant


def _layer_chain(ln=None, gemm=None, attn=None, quant=None):
    """The attention half with the restatements as the kernels; -> the violations of the GPU test's five stage checks."""
    from tests import attn_prefill_oracle as O

    L = C.layer_inputs()
    x0, s0 = C.ln_stand_in(L["ln"], ln)
    c1 = dict(x=x0, w=L["wqkv"], ws=L["ws_qkv"], as_=s0, bias=L["b_qkv"])
    qkv = C.gemm_stand_in(c1, gemm)
    q, k, v = [t.reshape(L["bsz"], L["seqlen"], L["heads"], L["dh"]) for t in qkv.split(L["emb"], dim=-1)]
    a = O.attention(q, k, v, None, False, mutant=attn).to(torch.float32).to(torch.float16).reshape(L["m"], L["emb"])
    x1, s1 = C.quant_stand_in(a, quant)
    out = C.gemm_stand_in(dict(x=x1, w=L["wo"], ws=L["ws_o"], as_=s1, bias=L["b_o"]), gemm)
    return [C.ln_bound(x0, s0, L["ln"]), C.gemm_stage(qkv, x0, L["wqkv"], L["ws_qkv"], s0, L["b_qkv"]), C.attention_stage(a, qkv, L),
            C.quant_bits(x1, s1, a), C.gemm_stage(out, x1, L["wo"], L["ws_o"], s1, L["b_o"])]


def test_attention_half_checks_pass_the_oracle_and_see_faults():
    assert _layer_chain() == [{}, {}, {}, {}, {}]
    for mutant in ("rms", "nobeta_token"):
        assert _layer_chain(ln=mutant)[0] != {}, mutant
    r = _layer_chain(gemm="bias_first")
    assert r[1] != {} and r[4] != {}
    for mutant in ("kvh+1", "droptile"):  # four KV heads; 70 keys: the second tile holds six
        assert _layer_chain(attn=mutant)[2] != {}, mutant
    for mutant in ("trunc", "inv_from_scale"):
        assert _layer_chain(quant=mutant)[3] != {}, mutant
