"""not-gpu: the device-routing contract on the host -- the numpy oracle (tests/moe_route_oracle.py) against the torch glue it replaces, the C ABI's
argument validation (nothing is launched), and the module's `routing` argument."""
import ctypes

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi
from llm_awq_amd import moe as MOE
from tests import moe_route_oracle as R
from llm_awq_amd.qmodule import WQLinear
from tests.helpers import make_case, oracle_grouped_linear


def _experts(E, N, K, dtype, seed):
    mods = []
    for e in range(E):
        c = make_case(N, K, dtype, seed=seed + e)
        m = WQLinear(4, 128, K, N, False, "cpu", dtype=dtype)
        m.qweight, m.scales, m.scaled_zeros = c["qweight"], c["scales"], c["scaled_zeros"]
        mods.append(m)
    return mods


@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (65, 8, 2), (7, 64, 8), (130, 60, 4), (5, 1, 1), (9, 2, 2)])
def test_oracle_equals_topk_and_sort_by_expert_on_tie_free_inputs(T, E, k):
    logits = torch.from_numpy(R.lattice_logits(np.random.default_rng(T * 100 + E), T, E))
    ids, w, order, inv, offsets = R.route(logits, k)
    probs = torch.softmax(logits.float(), dim=-1)
    tw, tids = torch.topk(probs, k, dim=-1)
    assert np.array_equal(ids, tids.numpy()) and np.array_equal(ids, torch.topk(logits, k, dim=-1)[1].numpy())
    torder, toff = MOE.sort_by_expert(tids, E)
    assert np.array_equal(order, torder.numpy()) and order.dtype == np.int32
    assert np.array_equal(offsets, toff.numpy()) and offsets[-1] == T * k
    assert np.array_equal(inv[order], np.arange(T * k))
    # the glue's weights (fp32 softmax -> topk -> w / w.sum) are the oracle's up to fp32 rounding
    tw = (tw / tw.sum(-1, keepdim=True)).double().numpy()
    assert np.abs(tw / w - 1).max() < 1e-5
    w_plain = R.weights(R.logits_f32(logits), ids, renormalize=False)
    assert np.abs(torch.topk(probs, k, dim=-1)[0].double().numpy() / w_plain - 1).max() < 1e-5


def test_oracle_selection_with_ties_and_odd_bits():
    l = np.array([[1.0, 3.0, 3.0, -2.0], [0.0, -0.0, 0.0, -0.0], [-np.inf, -1.0, np.inf, -1.0], [5.0, 5.0, 5.0, 5.0]], dtype=np.float32)
    assert R.select(l, 3).tolist() == [[1, 2, 0], [0, 2, 1], [2, 1, 3], [0, 1, 2]]  # (+0 above -0 through the key; equal keys: lower index)
    k = R.float_key(np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dtype=np.float32)).astype(np.int64)
    assert (np.diff(k) > 0).all()
    w = R.weights(l[3:], R.select(l[3:], 2))
    assert w.tolist() == [[0.5, 0.5]]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_oracle_combine_equals_the_glue_expression_for_two_experts(dtype):
    T, k, H = 37, 2, 24
    g = torch.Generator().manual_seed(11)
    ys = torch.randn(T * k, H, generator=g).to(dtype)
    w32 = torch.rand(T, k, generator=g) + 0.01
    w32 = w32 / w32.sum(-1, keepdim=True)
    order = torch.randperm(T * k, generator=g)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(T * k)
    out = torch.zeros(T * k, H, dtype=dtype)
    out[order] = ys
    glue = (out.view(T, k, -1) * w32.to(dtype).unsqueeze(-1)).sum(1)
    got = R.combine(ys, inv.numpy().astype(np.int32), w32.numpy())
    assert torch.equal(got.view(torch.int16), glue.view(torch.int16))
    assert torch.equal(R.gather(ys, order.numpy().astype(np.int32), 1), ys[order])


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    SHAPE, ALIGN, NULL, DTYPE = -4, -5, -6, -3

    def route(T=4, E=8, k=2, dt=2, logits=p, ids=p, w=p, order=p, inv=p, off=p):
        return L.awq_moe_route(logits, dt, T, E, k, 1, ids, w, order, inv, off, None)

    assert route(E=0) == SHAPE and route(E=65) == SHAPE
    assert route(k=0) == SHAPE and route(E=4, k=5) == SHAPE and route(E=64, k=9) == SHAPE
    assert route(T=0) == SHAPE and route(T=(1 << 19) + 1, k=2) == SHAPE and route(T=(1 << 20) + 1, k=1) == SHAPE
    for name in ("logits", "ids", "w", "order", "inv", "off"):
        assert route(**{name: None}) == NULL, name
        assert route(**{name: p + 1}) == ALIGN, name
    assert route(dt=2, logits=p + 2) == ALIGN and route(dt=1, logits=p + 1) == ALIGN and route(dt=0, logits=p + 3) == ALIGN
    assert route(dt=3) == DTYPE and route(dt=-1) == DTYPE

    def gather(T=4, k=2, H=64, dt=1, x=p, order=p, xs=p):
        return L.awq_moe_gather(x, order, xs, T, k, H, dt, None)

    def combine(T=4, k=2, H=64, dt=1, ys=p, inv=p, w=p, out=p):
        return L.awq_moe_combine(ys, inv, w, out, T, k, H, dt, None)

    for fn, ptrs16, ptrs4 in ((gather, ("x", "xs"), ("order",)), (combine, ("ys", "out"), ("inv", "w"))):
        assert fn(T=0) == SHAPE and fn(k=0) == SHAPE and fn(k=9) == SHAPE and fn(T=(1 << 19) + 1) == SHAPE
        assert fn(H=0) == SHAPE and fn(H=12) == SHAPE
        assert fn(dt=2) == DTYPE and fn(dt=7) == DTYPE
        for name in ptrs16 + ptrs4:
            assert fn(**{name: None}) == NULL, name
        for name in ptrs16:
            assert fn(**{name: p + 8}) == ALIGN, name
        for name in ptrs4:
            assert fn(**{name: p + 2}) == ALIGN, name


def test_routing_argument():
    dtype, E, H, F = torch.bfloat16, 2, 128, 128
    w1, w3, w2 = (oracle_grouped_linear(_experts(E, n, k, dtype, s)) for n, k, s in ((F, H, 1), (F, H, 2), (H, F, 3)))
    with pytest.raises(ValueError):
        MOE.SparseMoeMLP(w1, w3, w2, 2, routing="bogus")
    m1 = _experts(E, F, H, dtype, 1)
    with pytest.raises(ValueError):
        MOE.SparseMoeMLP.fused(m1, m1, w2, 2, routing="bogus")
    assert MOE.SparseMoeMLP(w1, w3, w2, 2).routing == "torch" and MOE.SparseMoeMLP.fused(m1, m1, w2, 2).routing == "torch"
    blk = MOE.SparseMoeMLP(w1, w3, w2, 2, routing="device")
    x, logits = torch.zeros(3, H, dtype=dtype), torch.zeros(3, E)
    with pytest.raises(_capi.AwqNativeError):
        blk(x, logits)
    from llm_awq_amd import ops
    with pytest.raises(_capi.AwqNativeError):
        ops.moe_route(logits, 2)
    with pytest.raises(_capi.AwqNativeError):
        ops.moe_gather(x, torch.zeros(6, dtype=torch.int32), 2)
    with pytest.raises(_capi.AwqNativeError):
        ops.moe_combine(torch.zeros(6, H, dtype=dtype), torch.zeros(6, dtype=torch.int32), torch.zeros(3, 2))
