"""gpu: awq_moe_route_scored / ops.moe_route_scored / SparseMoeMLP(router=...) against a float64 numpy statement of the contract (`ref_route`:
include/awq_cdna4.h, DESIGN.md "MoE routing, scored"), against the old entry where both serve a shape, and against its own replay in a hipGraph.

Inputs.  Every row of logits is a random permutation of E distinct lattice values in [-4, 4]: multiples of 1/32 (257 values) up to E = 257,
multiples of 1/64 (513 values, still exact in bf16 and fp16) for E = 384 and 512, which the coarser lattice cannot fill with distinct values.
A bias holds multiples of 1/128 in [-0.5, 0.5].

Near ties.  With a bias the device compares fp32 keys and the reference float64 ones.  A row is DECIDED when every gap between consecutive keys of
ranks 1 .. k + 1 among the kept experts, and the gap between the last kept and the first dropped group score, exceed GAP = 2e-6 (a few fp32
roundings of 2^-24 relative on values <= 4, with margin).  Ids and weights are compared on decided rows; at most 1 % of a case's rows may be
undecided, none when T < 100.  Without a bias the keys are the lattice logits and every row is decided.

Weight bound, relative, against float64, derived as tests/test_gpu_moe_route.py derives its 1e-5 for 64 summed terms: fp32 eps = 6e-8; the
exponent's argument (at most 8 log2 e) is rounded once ~ 5e-7; exp, the divide, the sigmoid's add and the scale about 5 eps = 3e-7; a sum of n
terms <= n eps, where n is the case's own count -- k with renormalisation, E for a plain softmax, 0 for a plain sigmoid; 2x margin on top:
w_rel(n) = 2 (8e-7 + 6e-8 n), which is 9.3e-6 at n = 64."""
import numpy as np
import pytest
import torch

from llm_awq_amd import moe as MOE
from tests import moe_route_oracle as R
from tests.test_gpu_moe_route import _assert_valid_sort, _experts

GAP = 2e-6
CONFIGS = {  # name: (E, k, has_bias, router keywords)
    "qwen3": (128, 8, False, dict(score="softmax")),
    "dsv2": (160, 6, False, dict(score="softmax", renormalize=False, n_group=8, topk_group=3, scale=16.0)),
    "dsv3": (256, 8, True, dict(score="sigmoid", n_group=8, topk_group=4, group_top=2, scale=2.5)),
    "kimi": (384, 8, True, dict(score="sigmoid", scale=2.827)),
    "e65": (65, 8, False, dict(score="sigmoid")),      # the first count the old entry refuses; a ragged second slot
    "e512": (512, 8, False, dict(score="softmax")),
    "e8": (8, 2, False, dict(score="sigmoid", n_group=4, topk_group=1)),   # k = the kept set
}
TOKENS = [1, 64, 65, 203, 8193]   # the one-launch edge; 26 chunks of 8, the last one of 3; the first T with chunks of 9
CASES = [(c, torch.float32) for c in CONFIGS] + [(c, dt) for c in ("qwen3", "dsv3") for dt in (torch.bfloat16, torch.float16)]   # each at every T


def w_rel(n_terms):
    return 2 * (8e-7 + 6e-8 * n_terms)


def lattice(rng, T, E):
    n = 257 if E <= 257 else 513
    pick = np.argsort(rng.random((T, n)), axis=1)[:, :E]
    return ((pick - n // 2) * (8.0 / (n - 1))).astype(np.float32)


def make_bias(E, seed=0):
    return (np.random.default_rng(9000 + seed).integers(-64, 65, E) / 128.0).astype(np.float32)


def ref_route(l32, k, score="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, group_top=1, scale=1.0):
    """the contract in float64 -> (ids int32 [T, k], w float64 [T, k], decided bool [T])"""
    l = l32.astype(np.float64)
    T, E = l.shape
    with np.errstate(all="ignore"):
        if score == "softmax":
            ex = np.exp(l - l.max(1, keepdims=True))
            s = ex / ex.sum(1, keepdims=True)
        else:
            s = 1.0 / (1.0 + np.exp(-l))
        key = l if bias is None else s + bias.astype(np.float64)
        decided = np.ones(T, dtype=bool)
        if n_group > 1:
            gscore = -np.sort(-key.reshape(T, n_group, -1), axis=2)[:, :, :group_top].sum(2)
            gorder = np.argsort(-gscore, axis=1, kind="stable")
            gsorted = np.take_along_axis(gscore, gorder, 1)
            if topk_group < n_group:
                decided &= gsorted[:, topk_group - 1] - gsorted[:, topk_group] > GAP
            keep = np.zeros((T, n_group), dtype=bool)
            np.put_along_axis(keep, gorder[:, :topk_group], True, 1)
            key = np.where(np.repeat(keep, E // n_group, axis=1), key, -np.inf)
        order = np.argsort(-key, axis=1, kind="stable")
        ranked = np.take_along_axis(key, order[:, :k + 1], 1)
        decided &= (ranked[:, :-1] - ranked[:, 1:] > GAP).all(1) if ranked.shape[1] > 1 else True
        ids = order[:, :k]
        w = np.take_along_axis(s, ids, 1)
        if renormalize:
            w = w / (w.sum(1, keepdims=True) + 1e-20)
    return ids.astype(np.int32), w * scale, decided


@pytest.fixture(scope="module")
def ops():
    from llm_awq_amd import ops as o
    return o


def _case(name, T, seed=0):
    E, k, has_bias, kw = CONFIGS[name]
    l = lattice(np.random.default_rng(100000 * seed + 10 * T + E), T, E)
    return l, k, (make_bias(E, seed) if has_bias else None), kw


def _route(ops, logits, k, bias, kw):
    b = None if bias is None else torch.from_numpy(bias).cuda()
    out = ops.moe_route_scored(logits.cuda(), k, bias=b, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_sorted_own_ids(got, E, what):
    ids, _w, order, inv, off = got
    so, si, sf = R.sort_slots(ids, E)
    assert np.array_equal(order, so) and np.array_equal(inv, si) and np.array_equal(off, sf), what


def _assert_equals_ref(got, ref, n_terms, what, rows=None):
    ids, w = got[0], got[1]
    rids, rw, decided = ref
    if rows is not None:
        decided = decided & np.isin(np.arange(len(decided)), rows)
    assert np.array_equal(ids[decided], rids[decided]), what
    rel = np.abs(w[decided].astype(np.float64) / rw[decided] - 1).max() if decided.any() else 0.0
    print(f"{what}: weights rel err {rel:.2e} (bound {w_rel(n_terms):.1e}), undecided rows {int((~ref[2]).sum())}")
    assert rel <= w_rel(n_terms), (what, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", CASES)
def test_route_equals_reference(ops, name, dtype):
    for T in TOKENS:
        l, k, bias, kw = _case(name, T)
        E = l.shape[1]
        logits = torch.from_numpy(l).to(dtype)
        got = _route(ops, logits, k, bias, kw)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == (T, k)
        ref = ref_route(R.logits_f32(logits), k, bias=bias, **kw)
        assert (~ref[2]).sum() <= (0 if T < 100 else T // 100), "too many near-tie rows: pick another seed"
        n_terms = k if kw.get("renormalize", True) else (E if kw["score"] == "softmax" else 0)
        _assert_equals_ref(got, ref, n_terms, f"{name} T={T} {dtype}")
        _assert_sorted_own_ids(got, E, f"{name} T={T} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("E,k,kw,want", [(128, 8, dict(score="softmax", scale=3.0), list(range(8))),
                                         (384, 5, dict(score="sigmoid", scale=0.5), list(range(5))),
                                         (256, 8, dict(score="sigmoid", n_group=8, topk_group=4, group_top=2, scale=2.5), list(range(8))),
                                         (160, 6, dict(score="softmax", n_group=8, topk_group=3), list(range(6))),
                                         (8, 2, dict(score="sigmoid", n_group=4, topk_group=1), [0, 1])])
def test_ties_take_the_lower_expert_and_the_lower_group(ops, E, k, kw, want):
    T = 67
    got = _route(ops, torch.full((T, E), 0.375), k, None, kw)
    assert np.array_equal(got[0], np.tile(np.array(want, dtype=np.int32), (T, 1)))
    assert np.abs(got[1].astype(np.float64) * k / kw.get("scale", 1.0) - 1).max() <= w_rel(k)
    _assert_sorted_own_ids(got, E, f"ties E={E}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,E,k", [(7, 64, 8), (130, 60, 4), (1025, 8, 2)])
def test_same_answer_as_the_old_entry(ops, T, E, k):
    logits = torch.from_numpy(R.lattice_logits(np.random.default_rng(T + E), T, E)).cuda()
    new, old = ops.moe_route_scored(logits, k, score="softmax"), ops.moe_route(logits, k)
    for i in (0, 2, 3, 4):
        assert new[i].dtype == old[i].dtype and torch.equal(new[i], old[i]), i
    assert float((new[1].double() / old[1].double() - 1).abs().max()) <= w_rel(k)


@pytest.mark.gpu
def test_nan_and_minus_inf_rows_keep_the_indices_valid(ops):
    T = 70
    l, k, bias, kw = _case("dsv3", T, seed=1)
    E, bad = l.shape[1], [2, T // 2, T - 1]
    clean = _route(ops, torch.from_numpy(l), k, bias, kw)
    l = l.copy()
    l[bad[0], ::3] = np.nan
    l[bad[1], :] = -np.inf
    l[bad[2], :] = np.nan
    got = _route(ops, torch.from_numpy(l), k, bias, kw)
    _assert_valid_sort(got[0], got[2], got[3], got[4], T, E, k)
    _assert_sorted_own_ids(got, E, "robust")
    assert all(len(set((got[0][t] // (E // kw["n_group"])).tolist())) <= kw["topk_group"] for t in bad)
    good = np.setdiff1d(np.arange(T), bad)
    assert np.array_equal(got[0][good], clean[0][good]) and np.array_equal(got[1][good], clean[1][good])
    ref = ref_route(np.where(np.isfinite(l), l, 0).astype(np.float32), k, bias=bias, **kw)
    assert ref[2][good].all(), "a near-tie row: pick another seed"
    _assert_equals_ref(got, ref, k, "robust", rows=good)


# ---- the block: E = 72 is the first grouped launch above the 64-expert tail switch ----
E_BLK, H_BLK, F_BLK, K_BLK, DT_BLK = 72, 256, 512, 8, torch.bfloat16


@pytest.fixture(scope="module")
def block():
    m1, m3, m2 = _experts(E_BLK, F_BLK, H_BLK, DT_BLK, 1310), _experts(E_BLK, F_BLK, H_BLK, DT_BLK, 1510), _experts(E_BLK, H_BLK, F_BLK, DT_BLK, 1710)
    bias = make_bias(E_BLK)
    bias[3] = -0.5   # with logit -100 expert 3's key is the smallest possible one: the replay test empties it
    router = MOE.MoeRouter("sigmoid", True, torch.from_numpy(bias).cuda(), n_group=8, topk_group=4, group_top=2, scale=2.5)
    blk = MOE.SparseMoeMLP.fused(m1, m3, MOE.GroupedWQLinear(m2).cuda().to_cdna4(), K_BLK, routing="device", router=router)
    blk.gate_up.cuda()
    return blk


def _block_inputs(T, seed):
    x = torch.randn(T, H_BLK, generator=torch.Generator().manual_seed(seed)).to(DT_BLK).cuda()
    return x, torch.from_numpy(lattice(np.random.default_rng(seed), T, E_BLK)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 9, 130])
def test_block_is_the_composition_of_its_launches(ops, block, T):
    x, logits = _block_inputs(T, 50 + T)
    y = block(x, logits)
    _ids, w, order, _inv, off = ops.moe_route_scored(logits, K_BLK, **block.router.kwargs())
    xs = x[(order // K_BLK).long()]
    ys = block.w2(block._h(xs, off), off)
    out = torch.zeros(T * K_BLK, ys.shape[1], dtype=ys.dtype, device=ys.device)
    out[order.long()] = ys
    want = R.combine(out.cpu(), np.arange(T * K_BLK, dtype=np.int32), w.cpu().numpy())   # (more than two experts: the fp32 sum of the contract)
    assert y.shape == (T, H_BLK) and y.dtype == DT_BLK and float(y.float().abs().max()) > 0
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [9, 130])   # the one-launch form, and the three launches with their workspace
def test_block_replays_in_a_graph(ops, block, T):
    x_s, l_s = _block_inputs(T, 7)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block(x_s, l_s)  # warm-up (allocator pools, the side buffers of the grouped modules)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = block(x_s, l_s)
    for step in range(2):
        x_n, l_n = _block_inputs(T, 200 + step)
        if step == 1:
            l_n[:, 3] = -100.0
        x_s.copy_(x_n)
        l_s.copy_(l_n)
        graph.replay()
        y_e = block(x_n.clone(), l_n.clone())
        off = ops.moe_route_scored(l_n, K_BLK, **block.router.kwargs())[4]
        torch.cuda.synchronize()
        assert torch.equal(y_g.view(torch.int16), y_e.view(torch.int16)), step
        assert step == 0 or int(off[4] - off[3]) == 0, "expert 3 was to stay empty"


@pytest.mark.gpu
def test_extension_export_equals_ops_and_both_refuse(ops):
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    l, k, bias, kw = _case("dsv3", 203)
    logits, b = torch.from_numpy(l).to(torch.bfloat16).cuda(), torch.from_numpy(bias).cuda()
    a, e = ops.moe_route_scored(logits, k, bias=b, **kw), eng.moe_route_scored(logits, k, bias=b, **kw)
    assert len(e) == 5 and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, e))
    for E, kk, bad in ((513, 8, {}), (128, 9, {}), (128, 8, dict(score="softmax", bias=torch.zeros(128).cuda())), (128, 8, dict(n_group=3, topk_group=3))):
        with pytest.raises(ValueError):
            ops.moe_route_scored(torch.zeros(4, E).cuda(), kk, **bad)
        with pytest.raises(RuntimeError):
            eng.moe_route_scored(torch.zeros(4, E).cuda(), kk, **bad)
