"""-m gpu: the split-K path of the narrow-tile prefill GEMM (awq_gemm_v4n.hip) -- prompts of 256 .. ~1 k tokens against
projections whose output tiles fill less than half of the chip.  The K ranges are summed in fp32 in a fixed order, so the
result is deterministic but not bit-identical to the unsplit kernel (a different association of the same fp32 products);
both must sit within the reference tolerance of a torch fp32 matmul on the dequantised weights.  The reference's own
split-K (gemm_cuda.cu:546-619) has the same property."""
import pytest
import torch

from tests.helpers import assert_bits, cuda_gen, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _poison():
    """uninitialised outputs and workspaces are NaN-filled (helpers.poisoned): a second call cannot pass on the first call's freed block"""
    with poisoned():
        yield


SHAPES = [(4096, 4096), (14336, 4096), (1024, 1296), (4096, 6144), (8192, 1024)]


@pytest.fixture(scope="module")
def env():
    from llm_awq_amd import ops, synth
    ops._capi.lib()
    return ops, synth


def test_workspace_query(env):
    ops, _ = env
    L = ops._capi.lib()
    q = L.awq_w4a16_forward_cdna4_workspace_bytes
    assert q(1, 4096, 4096) == 0 and q(16, 4096, 4096) == 0 and q(32, 4096, 4096) == 0   # GEMV / skinny with a full grid against a short K: no workspace
    # skinny launches that leave half the chip idle: two K parts of fp32 sums, [2][rows of a pass][n] (33..64 rows from K = 4096, 17..32 rows from K = 8192)
    assert q(64, 4096, 4096) == 2 * 64 * 4096 * 4 and q(40, 4096, 14336) == 2 * 40 * 4096 * 4 and q(24, 4096, 14336) == 2 * 24 * 4096 * 4
    assert q(64, 6144, 4096) == 0                                  # (384 slabs: two parts would be 1.5 rounds of blocks)
    assert q(71, 4096, 8192) == 8 * 71 * 4096 * 4                  # 65 .. 128 rows: the mid-M kernel's parts (tests/test_gpu_midm.py): 32 slab groups x 8 parts of 8 k-steps
    assert q(64, 28672, 8192) == 0 and q(32, 8192, 8192) == 0                                   # wide N fills the chip unsplit
    assert q(64, 8192, 8192) % (64 * 8192 * 4) == 0 and q(64, 8192, 8192) >= 2 * 64 * 8192 * 4   # (33 .. 64 rows against n = 8192: the mid-M kernel's K split, round 6)
    tile = 256 * 128 * 4                                            # one fp32 partial tile
    for (m, n, k, tiles) in ((256, 4096, 14336, 32), (512, 4096, 4096, 64)):
        b = q(m, n, k)
        assert b > 0 and b % (tiles * tile) == 0 and 2 <= b // (tiles * tile) <= 16, (m, n, k, b)
    ops._capi.tune(gemm_splitk=5)                                   # experiments: a forced number of K ranges
    try:
        assert q(256, 4096, 14336) == 32 * 5 * tile
    finally:
        ops._capi.tune(gemm_splitk=1)
    assert q(256, 4096, 4096 + 64) == 0                            # K not a multiple of 128: not this path
    ops._capi.tune(gemm_splitk=0)
    try:
        assert q(256, 4096, 14336) == 0
    finally:
        ops._capi.tune(gemm_splitk=1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K,N", SHAPES)
def test_splitk_vs_unsplit_and_torch_fp32(env, dtype, K, N):
    ops, synth = env
    L = ops._capi.lib()
    w = synth.random_wq(K, N, dtype=dtype, seed=K + 3 * N, keep_q=False)
    c4 = ops.repack_v2_to_cdna4(w["qweight"])
    szp = ops.pack_sz_cdna4(w["scales"], w["scaled_zeros"], K)
    W = ops.dequant_cdna4(c4, w["scales"], w["scaled_zeros"]).float()
    g = cuda_gen(5)
    bias = (torch.randn(N, device="cuda", generator=g) * 0.02).to(dtype)
    split_seen = 0
    for M in (256, 300, 512, 777, 1024):
        x = torch.randn(M, K, device="cuda", generator=g).to(dtype)
        for b in (None, bias):
            ref = (x.float() @ W.t()).to(dtype)
            if b is not None:
                ref = ref + b
            ops._capi.tune(gemm_splitk=0)
            y0 = ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], b, szp)
            for knob in (1, 3, 5):  # auto; forced 3 / 5 K ranges (uneven ranges when K/128 is not a multiple)
                ops._capi.tune(gemm_splitk=knob)
                try:
                    split = L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K) > 0
                    y = ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], b, szp)
                    y2 = ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], b, szp)
                finally:
                    ops._capi.tune(gemm_splitk=1)
                split_seen += split
                assert torch.equal(y, y2), (M, knob, "split-K must be deterministic")
                if not split:
                    assert torch.equal(y, y0), (M, knob)
                for name, v in (("split", y), ("unsplit", y0)):
                    rel = ((v.float() - ref.float()).norm() / ref.float().norm()).item()
                    assert rel < 1e-3, (name, M, knob, rel)
                    assert_bits(ref, v, 0.03, what=str((name, M, knob)))
                assert_bits(y, y0, 0.03, what=str((M, knob)))
                assert ((y.float() - y0.float()).norm() / y0.float().norm()).item() < 1e-3, (M, knob)
    assert split_seen >= 10, "the split path was not exercised"


def test_splitk_without_workspace_runs_unsplit(env):
    """The workspace is optional in the C ABI: a call without it gives the unsplit kernel's bits."""
    ops, synth = env
    L = ops._capi.lib()
    K, N, M = 4096, 4096, 512
    w = synth.random_wq(K, N, dtype=torch.bfloat16, seed=9, keep_q=False)
    c4 = ops.repack_v2_to_cdna4(w["qweight"])
    szp = ops.pack_sz_cdna4(w["scales"], w["scaled_zeros"], K)
    x = torch.randn(M, K, device="cuda").bfloat16()
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops._capi.check(L.awq_w4a16_forward_cdna4(x.data_ptr(), c4.data_ptr(), w["scales"].data_ptr(), w["scaled_zeros"].data_ptr(),
                                              szp.data_ptr(), None, out.data_ptr(), M, N, K, 128, 1, None, 0, None))
    torch.cuda.synchronize()
    ops._capi.tune(gemm_splitk=0)
    try:
        y0 = ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], None, szp)
    finally:
        ops._capi.tune(gemm_splitk=1)
    assert torch.equal(out, y0)


def test_splitk_through_the_engine_and_graph(env):
    """awq_inference_engine.gemm_forward_cuda_new allocates the workspace itself; replaying it from a HIP graph works."""
    ops, synth = env
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    eng.cdna4_cache_enable(True)
    K, N, M = 4096, 4096, 512
    w = synth.random_wq(K, N, dtype=torch.bfloat16, seed=21, keep_q=False)
    x = torch.randn(M, K, device="cuda").bfloat16()
    y = eng.gemm_forward_cuda_new(x, w["qweight"], w["scales"], w["scaled_zeros"])  # warms the repack cache
    c4 = ops.repack_v2_to_cdna4(w["qweight"])
    szp = ops.pack_sz_cdna4(w["scales"], w["scaled_zeros"], K)
    assert torch.equal(y, ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], None, szp))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.gemm_forward_cuda_new(x, w["qweight"], w["scales"], w["scaled_zeros"])
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = eng.gemm_forward_cuda_new(x, w["qweight"], w["scales"], w["scaled_zeros"])
    x.copy_(torch.randn(M, K, device="cuda").bfloat16())
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], None, szp))


# ---------------- prompts shorter than one 256-row tile on the prefill GEMM (masked rows) ----------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [9, 33, 100, 129, 255])
@pytest.mark.parametrize("N,K", [(768, 3072), (144, 1280)])
def test_small_m_gemm_vs_oracle(env, dtype, M, N, K):
    """knob gemm_small_m=2 sends every 9 <= m <= 255 to awq_gemm_v4n.hip's single row tile: rows >= m are computed from
    row m - 1 and not stored (the guard rows around `out` must stay untouched), split-K on or off."""
    from tests.helpers import check_forward, make_case, cuda_gen, assert_bits
    ops, _ = env
    c = make_case(N, K, dtype, seed=M + N + K, M=M, bias=(M % 2 == 1))
    c4 = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    bias = c["bias"].cuda() if c["bias"] is not None else None
    for splitk in (1, 0, 3):
        ops._capi.tune(gemm_small_m=2, gemm_splitk=splitk)
        try:
            y = ops.gemm_cdna4(c["x"].cuda(), c4, c["scales"].cuda(), c["scaled_zeros"].cuda(), bias).cpu()
        finally:
            ops._capi.tune(gemm_small_m=1, gemm_splitk=1)
        check_forward(y, c["x"], c["q"], c["scales"], c["scaled_zeros"], dtype, bias=c["bias"])


def test_small_m_gemm_writes_only_its_rows(env):
    ops, synth = env
    L = ops._capi.lib()
    K, N = 4096, 4096
    w = synth.random_wq(K, N, dtype=torch.bfloat16, seed=77, keep_q=False)
    c4 = ops.repack_v2_to_cdna4(w["qweight"])
    szp = ops.pack_sz_cdna4(w["scales"], w["scaled_zeros"], K)
    W = ops.dequant_cdna4(c4, w["scales"], w["scaled_zeros"]).float()
    for M in (96, 200):
        for knob in (2, 1):
            ops._capi.tune(gemm_small_m=knob)
            try:
                x = torch.randn(M, K, device="cuda").bfloat16()
                buf = torch.full((M + 64, N), 7.0, device="cuda", dtype=torch.bfloat16)  # guard rows after the output
                wsb = L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K)
                ws = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device="cuda")
                ops._capi.check(L.awq_w4a16_forward_cdna4(x.data_ptr(), c4.data_ptr(), w["scales"].data_ptr(), w["scaled_zeros"].data_ptr(),
                                                          szp.data_ptr(), None, buf.data_ptr(), M, N, K, 128, 1,
                                                          ws.data_ptr() if wsb else None, wsb, None))
                torch.cuda.synchronize()
            finally:
                ops._capi.tune(gemm_small_m=1)
            assert torch.all(buf[M:] == 7.0), (M, knob)
            ref = (x.float() @ W.t()).bfloat16()
            rel = ((buf[:M].float() - ref.float()).norm() / ref.float().norm()).item()
            assert rel < 1e-3, (M, knob, rel)
            assert_bits(ref, buf[:M], 0.03, what=str((M, knob)))


def test_small_m_rule(env):
    """The round-5 rule (knob midm = 0; the default hands 65 .. 192 rows to the mid-M kernel): the GEMM takes m >= 256, and shorter prompts only where its
    256-row tile beats the skinny kernel."""
    ops, _ = env
    q = ops._capi.lib().awq_w4a16_forward_cdna4_workspace_bytes
    ops._capi.tune(midm=0)
    try:
        assert q(128, 4096, 14336) > 0 and q(71, 4096, 14336) == 2 * 36 * 4096 * 4 < q(72, 4096, 14336)  # K = 14336: from 72 rows (below: the skinny launch's two K parts)
        assert q(128, 4096, 4096) == 2 * 64 * 4096 * 4 < q(192, 4096, 4096)   # K = 4096: from 147 rows
    finally:
        ops._capi.tune(midm=1)


# ---- the skinny launch's K split across blocks (awq_skinny_cdna4.hip: skinny_splitk_kernel; N = 4096 at 33..64 rows per pass) ----

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K,N", [(4096, 4096), (14336, 4096), (2048, 1040), (1024, 4096), (4096, 6144)])
def test_skinny_split_k_vs_oracle_and_unsplit(env, dtype, K, N):
    """two (or, forced, four) blocks per slab group each sum a K part; the block that draws the group's last ticket adds the parts in part order, rounds
    once and adds the bias.  Against the oracle's forward bound, deterministic from call to call, and close to the unsplit launch (another association)."""
    from oracle import awq_oracle as O  # noqa: F401
    from tests.helpers import check_forward, make_case
    if dtype == torch.float16 and (K, N) in ((14336, 4096), (4096, 6144)):
        pytest.skip("fp16 on the other three shapes (the CPU oracle of these two takes 10 - 20 s per dtype)")
    ops, _ = env
    L = ops._capi.lib()
    c = make_case(N, K, dtype, seed=K + N, M=100, bias=True)
    qw = ops.repack_v2_to_cdna4(c["qweight"].cuda())
    s, z, b = c["scales"].cuda(), c["scaled_zeros"].cuda(), c["bias"].cuda()
    szp = ops.pack_sz_cdna4(s, z, K)
    for M in (17, 33, 100, 48, 64):  # (100 rows: the mid-M kernel by default -- its parts are tests/test_gpu_midm.py's; the by-shape assertions below are for the skinny row counts)
        x = c["x"][:M].contiguous()
        xg = x.cuda()
        outs = {}
        for knob in (-1, 0, 2, 4):
            ops._capi.tune(skinny_splitk=knob)
            try:
                rows = -(-M // -(-M // 64))
                parts = L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K) // (rows * N * 4)
                y = ops.gemm_cdna4(xg, qw, s, z, b if M != 48 else None, szp)
                y2 = ops.gemm_cdna4(xg, qw, s, z, b if M != 48 else None, szp)
            finally:
                ops._capi.tune(skinny_splitk=-1)
            assert torch.equal(y, y2), (M, knob)  # the parts are added in part order whichever block arrives last
            if knob != 0:  # (the unsplit launch has its own oracle tests: test_gpu_cdna4.py)
                check_forward(y.cpu(), x, c["q"], c["scales"], c["scaled_zeros"], dtype, bias=c["bias"] if M != 48 else None)
            outs[knob] = (y, parts)
        nit = K // 128
        if M <= 64 and N * 2 // 32 <= 272 and nit % 2 == 0 and nit // 2 >= 8:  # (65 rows and up: the mid-M kernel / the masked-tile GEMM)
            assert outs[-1][1] == (2 if (rows > 32 and nit >= 32) or nit >= 64 else 0), (M, outs[-1][1])  # by shape: 33..64 rows per pass from K = 4096, 17..32 rows from K = 8192
            assert outs[2][1] == 2 and outs[0][1] == 0
        assert_bits(outs[2][0], outs[0][0], 0.02, "two K parts vs unsplit")
        assert_bits(outs[4][0], outs[0][0], 0.02, "four K parts vs unsplit")


def test_skinny_split_k_graph_replay_and_no_workspace(env):
    """a captured split launch replays (the last block puts the ticket words back to 0), two split launches in one graph use their own ticket lanes;
    a caller without scratch gets the unsplit launch"""
    ops, synth = env
    L = ops._capi.lib()
    K, N, M, dtype = 8192, 4096, 64, torch.bfloat16
    w = synth.random_wq(K, N, dtype=dtype, seed=9, keep_q=False)
    c4 = ops.repack_v2_to_cdna4(w["qweight"])
    szp = ops.pack_sz_cdna4(w["scales"], w["scaled_zeros"], K)
    g = cuda_gen(11)
    xs = [torch.randn(M, K, device="cuda", generator=g).to(dtype) for _ in range(3)]
    ref = [ops.gemm_cdna4(x, c4, w["scales"], w["scaled_zeros"], None, szp) for x in xs]
    assert L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K) > 0
    xin, xin_b = xs[0].clone(), xs[0].clone()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            yg = ops.gemm_cdna4(xin, c4, w["scales"], w["scaled_zeros"], None, szp)
            yg2 = ops.gemm_cdna4(xin_b, c4, w["scales"], w["scaled_zeros"], None, szp)  # a second split launch in the same graph (its own ticket lane)
        for i, x in enumerate(xs):
            xin.copy_(x)
            xin_b.copy_(xs[(i + 1) % 3])
            graph.replay()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, ref[i]) and torch.equal(yg2, ref[(i + 1) % 3])
    # direct C-ABI call without scratch: unsplit
    out = torch.empty(M, N, dtype=dtype, device="cuda")
    ops._capi.check(L.awq_w4a16_forward_cdna4(xs[1].data_ptr(), c4.data_ptr(), w["scales"].data_ptr(), w["scaled_zeros"].data_ptr(), szp.data_ptr(), None,
                                              out.data_ptr(), M, N, K, 128, 1, None, 0, None))
    torch.cuda.synchronize()
    ops._capi.tune(skinny_splitk=0)
    try:
        unsplit = ops.gemm_cdna4(xs[1], c4, w["scales"], w["scaled_zeros"], None, szp)
    finally:
        ops._capi.tune(skinny_splitk=-1)
    assert torch.equal(out, unsplit)
