"""not-gpu: the scored-routing contract on the host -- the torch glue of SparseMoeMLP(routing="torch", router=...) against the float64 reference of
tests/test_gpu_moe_route_scored.py, and the C ABI's refusals and workspace rule (nothing is launched)."""
import ctypes

import numpy as np
import torch

from llm_awq_amd import _capi
from llm_awq_amd import moe as MOE
from tests import moe_route_oracle as R
from tests.helpers import oracle_grouped_linear, oracle_sparse_moe
from tests.test_gpu_moe_route_scored import lattice, make_bias, ref_route, w_rel
from tests.test_moe_route_host import _experts


def test_torch_glue_of_the_block_equals_the_reference():
    dtype, E, k, H, F, T = torch.bfloat16, 8, 2, 128, 128, 37
    kw = dict(score="sigmoid", renormalize=True, n_group=4, topk_group=2, group_top=2, scale=2.5)
    bias = make_bias(E)
    w1, w3, w2 = (oracle_grouped_linear(_experts(E, n, kk, dtype, s)) for n, kk, s in ((F, H, 1), (F, H, 20), (H, F, 40)))
    blk = oracle_sparse_moe(w1, w3, w2, k)
    blk.router = MOE.MoeRouter(bias=torch.from_numpy(bias), **kw)
    l = lattice(np.random.default_rng(5), T, E)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(5)).to(dtype)
    ids, w, decided = ref_route(l, k, bias=bias, **kw)
    assert decided.all(), "a near-tie row: pick another seed"
    tids, tw = blk.router.route_torch(torch.from_numpy(l), k)
    assert np.array_equal(tids.numpy(), ids) and np.abs(tw.double().numpy() / w - 1).max() <= w_rel(k)
    order, inv, off = R.sort_slots(ids, E)
    xs = R.gather(x, order, k)
    ys = blk.w2(blk._h(xs, torch.from_numpy(off)), torch.from_numpy(off))
    want = R.combine(ys, inv, w.astype(np.float32)).float()   # (two experts per token: the glue's expression is the contract's sum)
    y = blk(x, torch.from_numpy(l)).float()
    assert float((y - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()) and float(want.abs().max()) > 0


def test_c_abi_refusals_and_workspace_rule():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def route(T=4, E=128, k=8, score=1, bias=None, ng=1, tg=1, gt=1, ws=None, ws_bytes=0):
        return L.awq_moe_route_scored(p, 2, T, E, k, score, 1, bias, ng, tg, gt, 1.0, p, p, p, p, p, ws, ws_bytes, None)

    bad = [dict(E=513), dict(k=9), dict(E=4, k=5), dict(T=0), dict(T=(1 << 17) + 1), dict(score=2), dict(score=0, bias=p), dict(ng=3, tg=3),
           dict(ng=32, tg=32), dict(ng=8, tg=9), dict(E=64, ng=16), dict(ng=8, tg=4, gt=3), dict(score=0, ng=8, tg=4, gt=2),
           dict(E=8, k=2, ng=8, tg=4, gt=2)]
    assert [route(**b) for b in bad] == [-4] * len(bad) and route(bias=p + 1) == -5
    q = L.awq_moe_route_scored_workspace
    assert q(64, 512, 8) == 0 and q(65, 128, 8) == 9 * 128 * 4 and q(8192, 512, 8) == 1024 * 512 * 4 and q(8193, 512, 8) == 911 * 512 * 4
    assert route(T=65) == _capi.AWQ_ERR_WORKSPACE and route(T=65, ws=p, ws_bytes=q(65, 128, 8) - 1) == _capi.AWQ_ERR_WORKSPACE
