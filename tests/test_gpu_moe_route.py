"""gpu: MoE routing on the device (awq_moe_route / awq_moe_gather / awq_moe_combine and SparseMoeMLP(routing="device")) against the numpy oracle
of the contract (tests/moe_route_oracle.py), the torch glue it replaces, and its own replay inside a hipGraph.

Route inputs are lattice rows (a random permutation of E distinct multiples of 1/8 in [-4, 4]): exact in bf16 and fp16 and tie-free, so the integer
outputs must equal the oracle exactly.  Weight bound 1e-5 relative against float64: fp32 eps = 6e-8; the exponent's argument (at most 8 log2 e) is
rounded once ~ 5e-7; exp and the divide a few eps; a sum of at most 64 terms <= 4e-6; about 2x margin on top."""
import numpy as np
import pytest
import torch

from llm_awq_amd import moe as MOE
from llm_awq_amd.qmodule import WQLinear
from tests import moe_route_oracle as R
from tests.helpers import make_case

pytestmark = pytest.mark.gpu

W_REL = 1e-5
LOGIT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ROUTE_SHAPES = [(1, 8, 2), (3, 8, 2), (8, 8, 2),            # decode
                (63, 8, 2), (64, 8, 2), (65, 8, 2),         # wave edge
                (1023, 8, 2), (1025, 8, 2), (2048, 8, 2),   # round edge
                (7, 64, 8),                                 # both maxima
                (130, 60, 4), (5, 1, 1), (9, 2, 2)]         # ... and k = E


@pytest.fixture(scope="module")
def ops():
    from llm_awq_amd import ops as o
    return o


def _route(ops, logits, k, renormalize=True):
    out = ops.moe_route(logits.cuda(), k, renormalize=renormalize)
    torch.cuda.synchronize()
    ids, w, order, inv, off = (t.cpu().numpy() for t in out)
    assert ids.dtype == np.int32 and w.dtype == np.float32 and order.dtype == inv.dtype == off.dtype == np.int32
    return ids, w, order, inv, off


def _assert_route_equals_oracle(got, want, what, rows=None):
    ids, w, order, inv, off = got
    oids, ow, oorder, oinv, ooff = want
    sel = slice(None) if rows is None else rows
    assert np.array_equal(ids[sel], oids[sel]), what
    rel = np.abs(w[sel].astype(np.float64) / ow[sel] - 1).max()
    print(f"{what}: weights rel err {rel:.2e} (bound {W_REL:.0e})")
    assert rel <= W_REL, (what, rel)
    if rows is None:
        assert np.array_equal(order, oorder) and np.array_equal(inv, oinv) and np.array_equal(off, ooff), what


@pytest.mark.parametrize("renormalize", [True, False])
@pytest.mark.parametrize("dtype", LOGIT_DTYPES)
@pytest.mark.parametrize("T,E,k", ROUTE_SHAPES)
def test_route_equals_oracle(ops, T, E, k, dtype, renormalize):
    logits = torch.from_numpy(R.lattice_logits(np.random.default_rng(1000 * T + 10 * E + k), T, E)).to(dtype)
    got = _route(ops, logits, k, renormalize)
    _assert_route_equals_oracle(got, R.route(logits, k, renormalize), f"route T={T} E={E} k={k} {dtype} renorm={renormalize}")


@pytest.mark.parametrize("T", [5, 130, 1500])
def test_route_skewed_six_empty_experts(ops, T):
    """every token picks experts 5 and 2 (in either order) of eight: six empty groups, offsets repeat"""
    rng = np.random.default_rng(T)
    l = R.lattice_logits(rng, T, 8) / 4.0 - 2.0   # everything else in [-3, -1]
    first = rng.random(T) < 0.5
    l[:, 5] = np.where(first, 2.0, 1.5)
    l[:, 2] = np.where(first, 1.5, 2.0)
    logits = torch.from_numpy(l.astype(np.float32))
    got = _route(ops, logits, 2)
    _assert_route_equals_oracle(got, R.route(logits, 2), f"skewed T={T}")
    assert got[4].tolist() == [0, 0, 0, T, T, T, 2 * T, 2 * T, 2 * T]


@pytest.mark.parametrize("dtype", LOGIT_DTYPES)
@pytest.mark.parametrize("T,E,k", [(5, 8, 2), (3, 64, 8), (70, 3, 3), (4, 5, 1)])
def test_route_ties_take_the_lower_index_and_split_evenly(ops, T, E, k, dtype):
    logits = torch.full((T, E), 0.375).to(dtype)
    ids, w, order, inv, off = _route(ops, logits, k)
    assert np.array_equal(ids, np.tile(np.arange(k, dtype=np.int32), (T, 1)))
    assert (w == np.float32(1) / np.float32(k)).all(), w
    oids, _, oorder, oinv, ooff = R.route(logits, k)
    assert np.array_equal(ids, oids) and np.array_equal(order, oorder) and np.array_equal(inv, oinv) and np.array_equal(off, ooff)
    w_plain = _route(ops, logits, k, renormalize=False)[1]
    assert np.abs(w_plain.astype(np.float64) * E - 1).max() <= W_REL


def _assert_valid_sort(ids, order, inv, off, T, E, k):
    assert ids.min() >= 0 and ids.max() < E
    assert all(len(set(r)) == k for r in ids.tolist())
    assert np.array_equal(np.sort(order), np.arange(T * k)), "order is not a permutation"
    assert np.array_equal(inv[order], np.arange(T * k)), "inv is not the inverse of order"
    assert off[0] == 0 and off[-1] == T * k and (np.diff(off) >= 0).all()
    sorted_e = ids.reshape(-1)[order]
    assert (np.diff(sorted_e) >= 0).all()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(sorted_e, minlength=E))]))
    same = np.diff(sorted_e) == 0
    assert (np.diff(order)[same] > 0).all(), "not stable"


@pytest.mark.parametrize("dtype", LOGIT_DTYPES)
@pytest.mark.parametrize("T,E,k", [(70, 8, 2), (9, 64, 8), (1100, 8, 2)])
def test_route_nan_and_minus_inf_rows_keep_the_indices_valid(ops, T, E, k, dtype):
    """one row holds NaN, one is all -inf, one all NaN: their weights are unspecified, every integer output is still a valid sort, the other rows
    are what they are without them"""
    rng = np.random.default_rng(T + E)
    l = R.lattice_logits(rng, T, E)
    bad = [2, T // 2, T - 1] if T > 3 else [0]
    l[bad[0], ::3] = np.nan
    l[bad[1], :] = -np.inf
    l[bad[2], :] = np.nan
    if T > 8:
        l[5, 0] = np.inf   # (a +inf top logit: NaN weights, valid ids)
        bad.append(5)
    logits = torch.from_numpy(l).to(dtype)
    got = _route(ops, logits, k)
    ids, w, order, inv, off = got
    _assert_valid_sort(ids, order, inv, off, T, E, k)
    good = np.setdiff1d(np.arange(T), bad)
    clean = logits.clone()
    clean[bad] = 0.0
    _assert_route_equals_oracle(got, R.route(clean, k), f"robust T={T} E={E} k={k} {dtype}", rows=good)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k", [2, 3, 4, 8])
@pytest.mark.parametrize("H", [8, 136, 4096])
@pytest.mark.parametrize("T", [1, 5, 257])
def test_gather_and_combine_equal_oracle(ops, T, H, k, dtype):
    g = torch.Generator().manual_seed(T * 7919 + H * 13 + k)
    x = torch.randn(T, H, generator=g).to(dtype)
    ys = torch.randn(T * k, H, generator=g).to(dtype)
    w32 = torch.rand(T, k, generator=g) + 0.01
    w32 = (w32 / w32.sum(-1, keepdim=True)).contiguous()
    order = torch.randperm(T * k, generator=g).to(torch.int32)
    inv = torch.empty_like(order)
    inv[order.long()] = torch.arange(T * k, dtype=torch.int32)
    xs = ops.moe_gather(x.cuda(), order.cuda(), k).cpu()
    assert torch.equal(xs.view(torch.int16), R.gather(x, order.numpy(), k).view(torch.int16))
    out = ops.moe_combine(ys.cuda(), inv.cuda(), w32.cuda()).cpu()
    want = R.combine(ys, inv.numpy(), w32.numpy())
    assert out.shape == (T, H) and torch.equal(out.view(torch.int16), want.view(torch.int16))


def test_extension_exports_equal_ops(ops):
    """awq_inference_engine.moe_route / moe_gather / moe_combine (torch_binding.cpp) are the same C entries behind another binding"""
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    T, E, k, H = 70, 8, 2, 136
    logits = torch.from_numpy(R.lattice_logits(np.random.default_rng(3), T, E)).to(torch.bfloat16).cuda()
    g = torch.Generator().manual_seed(3)
    x, ys = torch.randn(T, H, generator=g).half().cuda(), torch.randn(T * k, H, generator=g).half().cuda()
    for renorm in (True, False):
        a, b = ops.moe_route(logits, k, renormalize=renorm), eng.moe_route(logits, k, renorm)
        assert len(b) == 5 and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))
    _ids, w, order, inv, _off = a
    assert torch.equal(ops.moe_gather(x, order, k), eng.moe_gather(x, order, k))
    assert torch.equal(ops.moe_combine(ys, inv, w), eng.moe_combine(ys, inv, w))
    with pytest.raises(RuntimeError):
        eng.moe_route(logits, 9, True)
    with pytest.raises(RuntimeError):
        eng.moe_gather(x.cpu(), order, k)


# ---- the block: the dimensions of tests/test_moe.py::test_gpu_sparse_moe_block_fused_equals_unfused ----
E_BLK, H_BLK, F_BLK, K_BLK, DT_BLK = 4, 256, 512, 2, torch.bfloat16


def _experts(E, N, K, dtype, seed):
    mods = []
    for e in range(E):
        c = make_case(N, K, dtype, seed=seed + e)
        m = WQLinear(4, 128, K, N, False, "cpu", dtype=dtype)
        m.qweight, m.scales, m.scaled_zeros = c["qweight"], c["scales"], c["scaled_zeros"]
        mods.append(m)
    return mods


@pytest.fixture(scope="module")
def blocks():
    """{kind: (routing='torch' block, routing='device' block)} sharing their expert modules"""
    m1, m3, m2 = _experts(E_BLK, F_BLK, H_BLK, DT_BLK, 310), _experts(E_BLK, F_BLK, H_BLK, DT_BLK, 320), _experts(E_BLK, H_BLK, F_BLK, DT_BLK, 330)
    w2 = MOE.GroupedWQLinear(m2).cuda().to_cdna4()
    fused_t = MOE.SparseMoeMLP.fused(m1, m3, w2, K_BLK)
    fused_t.gate_up.cuda()
    fused_d = MOE.SparseMoeMLP(None, None, w2, K_BLK, fused_t.gate_up, routing="device")
    w1, w3 = MOE.GroupedWQLinear(m1).cuda().to_cdna4(), MOE.GroupedWQLinear(m3).cuda().to_cdna4()
    return {"fused": (fused_t, fused_d), "plain": (MOE.SparseMoeMLP(w1, w3, w2, K_BLK), MOE.SparseMoeMLP(w1, w3, w2, K_BLK, routing="device"))}


def _block_inputs(T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H_BLK, generator=g).to(DT_BLK).cuda()
    logits = torch.from_numpy(R.lattice_logits(np.random.default_rng(seed), T, E_BLK)).cuda()
    return x, logits


@pytest.mark.parametrize("kind", ["fused", "plain"])
@pytest.mark.parametrize("T", [1, 4, 9, 130])
def test_block_device_routing_is_the_composition_of_its_launches(ops, blocks, kind, T):
    """routing="device" = moe_route's own outputs, a torch gather, the module's grouped launches and the glue's combine expression, bit for bit"""
    _, dev = blocks[kind]
    x, logits = _block_inputs(T, 50 + T)
    y = dev(x, logits)
    _ids, w, order, _inv, off = ops.moe_route(logits, K_BLK)
    xs = x[(order // K_BLK).long()]
    ys = dev.w2(dev._h(xs, off), off)
    out = torch.zeros(T * K_BLK, ys.shape[1], dtype=ys.dtype, device=ys.device)
    out[order.long()] = ys
    ref = (out.view(T, K_BLK, -1) * w.to(x.dtype).unsqueeze(-1)).sum(1)
    assert y.shape == (T, H_BLK) and y.dtype == DT_BLK
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))
    assert float(y.float().abs().max()) > 0


@pytest.mark.parametrize("kind", ["fused", "plain"])
@pytest.mark.parametrize("T", [1, 4, 9, 130])
def test_block_device_equals_torch_routing_on_even_weights(blocks, kind, T):
    """logits whose two largest entries per row are equal (2 at two random experts, distinct smaller lattice values elsewhere): both paths' weights
    are exactly 0.5, so the two routings must give the same bits"""
    tor, dev = blocks[kind]
    x, _ = _block_inputs(T, 90 + T)
    rng = np.random.default_rng(T)
    l = R.lattice_logits(rng, T, E_BLK) / 8.0 - 1.0   # distinct values in [-1.5, -0.5]
    for t in range(T):
        l[t, rng.permutation(E_BLK)[:2]] = 2.0
    logits = torch.from_numpy(l.astype(np.float32)).cuda()
    y_t, y_d = tor(x, logits), dev(x, logits)
    assert torch.equal(y_d.view(torch.int16), y_t.view(torch.int16))


def test_block_device_routing_replays_in_a_graph(blocks):
    """one captured forward, replayed on new contents that change the per-expert counts (one of them with an empty expert): each replay = the eager call"""
    _, dev = blocks["fused"]
    T = 9
    x_s, l_s = _block_inputs(T, 7)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dev(x_s, l_s)  # warm-up (allocator pools, the side buffers of the grouped modules)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = dev(x_s, l_s)
    counts = []
    for step in range(3):
        x_n, l_n = _block_inputs(T, 200 + step)
        if step == 1:
            l_n[:, 3] = -100.0  # expert 3 gets no token
        x_s.copy_(x_n)
        l_s.copy_(l_n)
        graph.replay()
        y_e = dev(x_n.clone(), l_n.clone())
        torch.cuda.synchronize()
        assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16)), step
        counts.append(np.diff(R.route(l_n, K_BLK)[4]).tolist())
    assert counts[1][3] == 0 and len({tuple(c) for c in counts}) == 3, counts
