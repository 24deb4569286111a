"""-m gpu: the decode entry point awq_w4a16_decode_cdna4 (LDS-DMA streaming kernel + f16-mantissa dequant, sz_half side buffer)
against the oracle: every row count 1..8, ragged K splits (11008 = 86 groups), tiny and wide shapes, bias, the fused gate/up
epilogues in both row arrangements, and the pack-time exactness check with its fallback."""
import numpy as np
import pytest
import torch

from oracle import awq_oracle as O
from tests.helpers import acc_slack, check_forward, check_fused_tail, make_case, assert_bits, weight_row_norms, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _poison():
    """uninitialised outputs and workspaces are NaN-filled (helpers.poisoned): a second call cannot pass on the first call's freed block"""
    with poisoned():
        yield


# norm-wise distance of the fused tail from the oracle's tail: BASELINE.json's 1e-3 (measured on MI355X: <= 3.7e-4 over every case of the suite,
# profiles/r05_test_stats.txt -- 2.7 x below it); the HARD criterion is check_fused_tail's elementwise hull
REL_TAIL = {torch.bfloat16: 1e-3, torch.float16: 1e-3}


@pytest.fixture(scope="module")
def ops():
    from llm_awq_amd import ops as o
    o._capi.lib()
    return o


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(16, 128), (48, 1280), (64, 11008), (256, 4096), (4096, 512), (6144, 4096), (4096, 14336)])
def test_pack_szh_matches_oracle_and_decode_vs_oracle(ops, dtype, N, K):
    if dtype == torch.float16 and N * K >= 6144 * 4096:
        pytest.skip("the two largest shapes in bf16 only (fp16: the five others)")
    c = make_case(N, K, dtype, seed=N + K, M=8, bias=True)
    s, z = c["scales"].cuda(), c["scaled_zeros"].cuda()
    szh, exact = ops.pack_szh_cdna4(s, z, K)
    ref, ref_exact = O.pack_sz_half(c["scales"], c["scaled_zeros"], K)
    assert exact and ref_exact
    assert np.array_equal(szh.cpu().numpy(), ref)
    c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    for M in (1, 2, 3, 4, 5, 7, 8):
        x = c["x"][:M].contiguous()
        for b in (None, c["bias"]):
            y = ops.decode_cdna4(x.cuda(), c4, szh, b.cuda() if b is not None else None, 0)
            check_forward(y.cpu(), x, c["q"], c["scales"], c["scaled_zeros"], dtype, bias=b)


def test_wide_launch_long_k_every_row_count(ops):
    """a wide launch (> 3 slabs per CU) against K = 8192 -- the class of Llama-3-70B's gate / up pair: the streaming kernel's eight-wave blocks at one row, the
    skinny kernel from two (round 6: the hand-over follows the bytes three co-resident blocks would stage), every row count against the oracle computed once"""
    from tests.helpers import check_forward_rows, forward_oracle
    N, K, dtype = 12320, 8192, torch.bfloat16   # 770 slabs = 3.008 per CU
    L = ops._capi.lib()
    import ctypes
    kern = ctypes.c_int(-1)
    assert [(L.awq_w4a16_decode_cdna4_plan(m, N, K, 0, ctypes.byref(kern)), kern.value) for m in (1, 2, 3, 8)] == [(1, 0), (1, 1), (1, 1), (1, 1)]
    c = make_case(N, K, dtype, seed=11, M=8, bias=True)
    szh, exact = ops.pack_szh_cdna4(c["scales"].cuda(), c["scaled_zeros"].cuda(), K)
    assert exact
    c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    pre = forward_oracle(c["x"], c["q"], c["scales"], c["scaled_zeros"], dtype, bias=c["bias"])
    for M in range(1, 9):
        y = ops.decode_cdna4(c["x"][:M].contiguous().cuda(), c4, szh, c["bias"].cuda(), 0)
        check_forward_rows(y.cpu(), pre, rows=M)


@pytest.mark.parametrize("knobs", [dict(gemvd_waves=4, gemvd_d=4), dict(gemvd_waves=8, gemvd_d=1), dict(gemvd_waves=8, gemvd_d=2), dict(gemvd_waves=8, gemvd_d=4), dict(gemvd_waves=8, gemvd_d=8),
                                   dict(gemvd_waves=16, gemvd_d=1), dict(gemvd_waves=16, gemvd_d=2), dict(gemvd_waves=16, gemvd_d=4)])
def test_decode_ring_configurations(ops, knobs):
    """every compiled (waves, ring depth) incl. ragged step counts, waves with no steps, and the counted tail waits"""
    try:
        for (N, K) in [(64, 11008), (128, 4096), (48, 1280), (32, 128), (32, 14336)]:
            for M in (1, 4, 8):
                c = make_case(N, K, torch.bfloat16, seed=N + M, M=M, bias=True)
                c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
                szh, exact = ops.pack_szh_cdna4(c["scales"].cuda(), c["scaled_zeros"].cuda(), K)
                assert exact
                ops._capi.tune(decode_skinny_from=9, **knobs)  # (9: every row count stays on the streaming kernel)
                y = ops.decode_cdna4(c["x"].cuda(), c4, szh, c["bias"].cuda(), 0)
                check_forward(y.cpu(), c["x"], c["q"], c["scales"], c["scaled_zeros"], torch.bfloat16, bias=c["bias"])
                # the same kernel on the T-typed sz_packed (the fallback for layers whose scales are not f16-exact)
                szp = ops.pack_sz_cdna4(c["scales"].cuda(), c["scaled_zeros"].cuda(), K)
                y2 = ops.gemm_cdna4(c["x"].cuda(), c4, c["scales"].cuda(), c["scaled_zeros"].cuda(), c["bias"].cuda(), szp)
                check_forward(y2.cpu(), c["x"], c["q"], c["scales"], c["scaled_zeros"], torch.bfloat16, bias=c["bias"])
                assert torch.equal(y, y2), "both dequant forms are exact: identical outputs"
    finally:
        ops._capi.tune(gemvd_waves=0, gemvd_d=0, decode_skinny_from=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("F,K", [(256, 768), (1376, 512), (64, 4096), (14336, 4096)])
def test_fused_gate_up_both_arrangements(ops, dtype, M, F, K):
    """epilogue 1 (stacked [gate; up]) and epilogue 2 (gate / up rows interleaved 8 + 8 per slab) == the reference's
    QuantLlamaMLP sequence (fused_mlp.py:36-83): two GEMVs, F.silu, multiply, every op rounded to T."""
    if F >= 4096 and (M not in (1, 8) or (M == 1 and dtype == torch.float16)):
        pytest.skip("full-size case: M = 1 (bf16) and 8 only")
    cg = make_case(F, K, dtype, seed=F + K + M, M=M)
    cu = make_case(F, K, dtype, seed=F + K + M + 1, M=M)
    x = cg["x"]
    g = O.wqlinear_forward(x, None, cg["scales"], cg["scaled_zeros"], None, 128, q_int=cg["q"])
    u = O.wqlinear_forward(x, None, cu["scales"], cu["scaled_zeros"], None, 128, q_int=cu["q"])
    ref = torch.nn.functional.silu(g) * u
    # stacked
    qgu = torch.cat([cg["qweight"], cu["qweight"]], 0).cuda()
    s = torch.cat([cg["scales"], cu["scales"]], 1).cuda()
    z = torch.cat([cg["scaled_zeros"], cu["scaled_zeros"]], 1).cuda()
    szh, exact = ops.pack_szh_cdna4(s, z, K)
    assert exact
    y1 = ops.decode_cdna4(x.cuda(), ops.repack_v2_to_cdna4(qgu), szh, None, 1).cpu()
    # interleaved: slab j = gate rows 8j..8j+7 then up rows 8j..8j+7 (packed v2 rows move in pairs: 4 logical rows each)
    from llm_awq_amd.fused_mlp import interleave_gate_up
    qi, si, zi = interleave_gate_up(cg["qweight"].cuda(), cu["qweight"].cuda(), cg["scales"].cuda(), cu["scales"].cuda(),
                                    cg["scaled_zeros"].cuda(), cu["scaled_zeros"].cuda())
    szh2, exact2 = ops.pack_szh_cdna4(si, zi, K)
    assert exact2
    y2 = ops.decode_cdna4(x.cuda(), ops.repack_v2_to_cdna4(qi), szh2, None, 2).cpu()
    for y in (y1, y2):
        check_fused_tail(y, g, u, REL_TAIL[dtype], what=f"decode gate/up F={F} K={K} M={M}", slack_g=acc_slack(x, weight_row_norms(cg)),
                         slack_u=acc_slack(x, weight_row_norms(cu)))
        assert_bits(y, ref, 0.05)
    assert_bits(y1, y2, 0.01)  # same math; only the split-K order inside a block differs


def test_inexact_scales_are_flagged(ops):
    """a bf16 scale below 2^-10 (s / 16 would be a subnormal f16) must be reported, and the T-typed path still serves it"""
    c = make_case(32, 256, torch.bfloat16, seed=5, M=2)
    s = c["scales"].clone()
    s[0, 3] = 2.0 ** -12
    sz = c["scaled_zeros"].clone()
    sz[0, 3] = -(s[0, 3].float() * 7).to(torch.bfloat16)
    szh, exact = ops.pack_szh_cdna4(s.cuda(), sz.cuda(), 256)
    assert not exact and not O.pack_sz_half(s, sz, 256)[1]
    c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    szp = ops.pack_sz_cdna4(s.cuda(), sz.cuda(), 256)
    y = ops.gemm_cdna4(c["x"].cuda(), c4, s.cuda(), sz.cuda(), None, szp)
    check_forward(y.cpu(), c["x"], c["q"], s, sz, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(16, 128), (48, 1280), (64, 11008), (4096, 512), (6144, 4096), (16400, 256)])
def test_batched_decode_on_the_skinny_kernel(ops, dtype, N, K):
    """the decode entry with its rows handed to the skinny kernel (x through registers, shared by a block's slabs; knob
    decode_skinny_from): every row count, bias, both side-buffer forms, narrow and wide (two slabs per block, ragged last block)"""
    if dtype == torch.float16 and N * K >= 6144 * 4096:
        pytest.skip("the largest shape in bf16 only")
    c = make_case(N, K, dtype, seed=N + K + 2, M=8, bias=True)  # (the parity of N + K: shares the full-size oracle case of the test above)
    c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    szh, exact = ops.pack_szh_cdna4(c["scales"].cuda(), c["scaled_zeros"].cuda(), K)
    assert exact
    try:
        ops._capi.tune(decode_skinny_from=1)
        for M in range(1, 9):
            x = c["x"][:M].contiguous()
            for b in (None, c["bias"]):
                y = ops.decode_cdna4(x.cuda(), c4, szh, b.cuda() if b is not None else None, 0)
                check_forward(y.cpu(), x, c["q"], c["scales"], c["scaled_zeros"], dtype, bias=b)
    finally:
        ops._capi.tune(decode_skinny_from=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [1, 5, 8])
@pytest.mark.parametrize("F,K", [(256, 768), (1376, 512), (14336, 4096)])
def test_fused_gate_up_on_the_skinny_kernel(ops, dtype, M, F, K):
    """epilogue 2 (8 + 8 interleaved pair -> silu(gate) * up) on the skinny kernel == the streaming kernel's result up to the
    split-K order, and == the reference's QuantLlamaMLP sequence (fused_mlp.py:36-83)"""
    from llm_awq_amd.fused_mlp import interleave_gate_up
    cg = make_case(F, K, dtype, seed=F + K + M, M=M)
    cu = make_case(F, K, dtype, seed=F + K + M + 1, M=M)
    x = cg["x"]
    g = O.wqlinear_forward(x, None, cg["scales"], cg["scaled_zeros"], None, 128, q_int=cg["q"])
    u = O.wqlinear_forward(x, None, cu["scales"], cu["scaled_zeros"], None, 128, q_int=cu["q"])
    ref = torch.nn.functional.silu(g) * u
    qi, si, zi = interleave_gate_up(cg["qweight"].cuda(), cu["qweight"].cuda(), cg["scales"].cuda(), cu["scales"].cuda(),
                                    cg["scaled_zeros"].cuda(), cu["scaled_zeros"].cuda())
    szh, exact = ops.pack_szh_cdna4(si, zi, K)
    assert exact
    c4 = ops.repack_v2_to_cdna4(qi)
    try:
        ops._capi.tune(decode_skinny_from=9)
        y_dma = ops.decode_cdna4(x.cuda(), c4, szh, None, 2).cpu()
        ops._capi.tune(decode_skinny_from=1)
        y = ops.decode_cdna4(x.cuda(), c4, szh, None, 2).cpu()
    finally:
        ops._capi.tune(decode_skinny_from=0)
    check_fused_tail(y, g, u, REL_TAIL[dtype], what=f"skinny gate/up F={F} K={K} M={M}", slack_g=acc_slack(x, weight_row_norms(cg)),
                     slack_u=acc_slack(x, weight_row_norms(cu)))
    assert_bits(y, ref, 0.05)
    assert_bits(y, y_dma, 0.01)
