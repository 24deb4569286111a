"""Decode attention on the MI355X against inputs whose answer is known to the bit (tests/attn_cases.py): every case asserts
out.view(int16) == target.view(int16), nothing weaker.  tests/test_attention_needle_host.py proves on the CPU, for this same list
of parameter sets, that the float64 oracle alone returns those bits and that oracle-level faults do not.

The only bounded comparison is the rotated k that the kernel writes into the cache: one ulp of T plus the angle slack, the bound
of test_gpu_attention.test_cache_contract.  Everything else in the caches (NaN slots, rows >= B) is compared bit for bit."""
import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from tests import attn_cases as C
from tests import attn_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I16 = torch.int16


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine  # the reference's module name (tinychat/models/llama.py)

    return awq_inference_engine


def _engine_call(E, q, k, v, kc, vc, lens, alibi, kw):
    return E.single_query_attention(q, k, v, kc, vc, lens, alibi, kw["timestep"], kw["rotary_embedding_dim"], kw["rotary_base"],
                                    kw["rotary_scale"], kw["neox_rotary_style"])


def _assert_bits(case, call, out, what):
    tg = case.target(call)
    bad = (out.view(I16) != tg.view(I16)).any(-1)
    if bad.any():
        where = [(int(b), int(h), int(case.needles[call, b, h]), int((case.needles[call, b, h] - case.first[b]) // case.chunk))
                 for b, h in bad.nonzero()[:8].tolist()]
        raise AssertionError(f"{what} call {call}: {int(bad.sum())} of {bad.numel()} heads differ from the target row; "
                             f"(row, head, needle, split) = {where}; plan = {(case.splits, case.chunk)}")


def _assert_cache_contract(case, kc1, vc1, what):
    """kc1 / vc1: the caches after the call(s), on the CPU."""
    s = case.spec
    k_rot = torch.stack([A.rotate(case.k[b], case.T[b], case.rot, case.base, case.scale, case.neox) for b in range(s["B"])])
    if case.rot:
        for b in range(s["B"]):
            if case.T[b] == 0:
                continue  # (position 0: the rotation is the identity and k_rot is k, compared below to the bit)
            ti = case.T[b] % s["Lmax"]
            for kvh in range(s["Hkv"]):
                got = A.k_cache_rows(kc1, b, kvh, [ti])[0]
                err = (got.double() - k_rot[b, kvh].double()).abs()
                lim = A.ulp(k_rot[b, kvh].double(), case.dtype) + A.angle_slack(case.k[b, kvh], case.T[b], case.rot, case.base, case.scale, case.neox)
                assert (err <= lim).all(), (what, b, kvh, err.max().item())
                k_rot[b, kvh] = got  # within the bound: take the written value, the rest of the cache is compared to the bit
    ekc, evc = case.expected_caches(k_rot)
    assert torch.equal(kc1.view(I16), ekc.view(I16)), f"{what}: k_cache differs outside the contract"
    assert torch.equal(vc1.view(I16), evc.view(I16)), f"{what}: v_cache differs outside the contract"


@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_needles(spec):
    case = C.Case(spec)
    dk, dv, dkc, dvc = (x.to(DEV) for x in (case.k, case.v, case.kc, case.vc))
    dl = case.lens.to(DEV) if case.lens is not None else None
    da = case.alibi.to(DEV) if case.alibi is not None else None
    outs = [ops.single_query_attention(case.q(c).to(DEV), dk, dv, dkc, dvc, dl, da, **case.kw) for c in range(case.ncalls)]
    torch.cuda.synchronize()
    for c, out in enumerate(outs):
        _assert_bits(case, c, out.cpu(), "C ABI")
    _assert_cache_contract(case, dkc.cpu(), dvc.cpu(), "C ABI")
    # the installed awq_inference_engine entry on caches of its own: the first and the last call of the group
    E = _engine()
    dkc2, dvc2 = case.kc.to(DEV), case.vc.to(DEV)
    for c in sorted({0, case.ncalls - 1}):
        out = _engine_call(E, case.q(c).to(DEV), dk, dv, dkc2, dvc2, dl, da, case.kw)
        _assert_bits(case, c, out.cpu(), "engine")
    _assert_cache_contract(case, dkc2.cpu(), dvc2.cpu(), "engine")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_graph_replay_after_lengths_and_needles_change_in_place(dtype):
    """One captured launch, replayed after length_per_sample, q (the needles) and the cache contents were rewritten in place."""
    tag = str(dtype)[6:]
    specs = {s["name"]: s for s in C.CASES}
    variants = [C.Case(specs[f"lens-graph-{x}-{tag}"]) for x in ("a", "b")]
    a = variants[0]
    assert all(v.spec["t"] == a.spec["t"] and v.kc.shape == a.kc.shape for v in variants)
    assert variants[0].T != variants[1].T and not np.array_equal(variants[0].needles, variants[1].needles)
    E = _engine()
    st = dict(q=a.q(0).to(DEV), k=a.k.to(DEV), v=a.v.to(DEV), kc=a.kc.to(DEV), vc=a.vc.to(DEV), lens=a.lens.to(DEV))

    def call():
        return _engine_call(E, st["q"], st["k"], st["v"], st["kc"], st["vc"], st["lens"], None, a.kw)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up (allocator pools)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = call()
    for step, v in enumerate((variants[0], variants[1], variants[0], variants[1])):
        call_idx = step % v.ncalls
        for name, src in (("q", v.q(call_idx)), ("k", v.k), ("v", v.v), ("kc", v.kc), ("vc", v.vc), ("lens", v.lens)):
            st[name].copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits(v, call_idx, out_g.cpu(), f"graph replay {step}")
        _assert_cache_contract(v, st["kc"].cpu(), st["vc"].cpu(), f"graph replay {step}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cache_above_2_31_elements(dtype):
    """More than 2^31 elements per cache, the needles in the last batch row and KV head (the size_t index arithmetic).  Built on the
    device: a random +-1 background, code rows only at the needles and their one-bit neighbours."""
    p = C.LARGE
    assert p["B"] * p["Hkv"] * p["Lmax"] * p["Dh"] > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GiB of free device memory for two caches above 2^31 elements, {free / 2 ** 30:.1f} GiB are free")
    q, k, v, kc, vc, t, needles, target = C.build_large(DEV, dtype, **p)
    B, Hkv, G, Lmax = p["B"], p["Hkv"], p["G"], p["Lmax"]
    assert ops.attn_decode_plan(B, Hkv, p["Dh"], t, Lmax)[0] == 1
    ti = t % Lmax

    def sums():
        return (torch.stack([kc[b].view(I16).sum(dtype=torch.int64) for b in range(B)]),
                torch.stack([vc[b].view(I16).sum(dtype=torch.int64) for b in range(B)]))

    old_k, old_v = kc[:, :, :, ti, :].clone(), vc[:, :, ti, :].clone()
    before = sums()
    out = ops.single_query_attention(q, k, v, kc, vc, None, None, timestep=t)
    out_e = _engine().single_query_attention(q, k, v, kc, vc, None, None, t)
    torch.cuda.synchronize()
    for o, what in ((out, "C ABI"), (out_e, "engine")):
        assert torch.isfinite(o.float()).all()
        mine = o[B - 1, (Hkv - 1) * G:].cpu()
        bad = (mine.view(I16) != target.view(I16)).any(-1)
        assert not bad.any(), (what, [(int(h), int(needles[h])) for h in bad.nonzero().reshape(-1)])
    # the slot of the current token holds k / v in every (row, KV head); with the old slot put back, nothing else has moved
    assert torch.equal(kc[:, :, :, ti, :].reshape(B, Hkv, -1).view(I16), k.view(I16))
    assert torch.equal(vc[:, :, ti, :].view(I16), v.view(I16))
    kc[:, :, :, ti, :] = old_k
    vc[:, :, ti, :] = old_v
    after = sums()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
