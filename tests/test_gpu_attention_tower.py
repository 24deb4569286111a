"""Encoder-tower attention on the MI355X (csrc/awq_attn_tower_cdna4.hip): the needle cases of tests/attn_tower_cases.py bit for bit
through the names the vision towers import, random inputs against the float64 oracle under the derived elementwise bound of
tests/attn_prefill_oracle.py, the dense and the varlen form against each other, every q tile of the plan, determinism and graph replay."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_oracle as O
from tests import attn_tower_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A  # bit pattern of the rows the kernel must not write


def _flash():
    llm_awq_amd.install_as_flash_attn()
    from flash_attn import flash_attn_func
    from flash_attn.flash_attn_interface import flash_attn_varlen_qkvpacked_func  # internvit.py:20

    return flash_attn_func, flash_attn_varlen_qkvpacked_func


def _bits(t):
    return t.cpu().view(torch.int16)


def _same(out, target, what=""):
    got, want = _bits(out), _bits(target)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.fixture
def rows_knob():
    yield lambda r: _capi.tune(tower_rows=r)
    _capi.tune(tower_rows=0)


# ------------------------------------------------------------------------------------------------------------------------
# needle cases
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.DENSE, ids=C.case_id)
def test_dense_needles_bit_exact(spec):
    case = C.dense_case(spec)
    q, k, v = case.to(DEV)
    assert q.stride() == case.q.stride() and k.stride() == case.k.stride()
    out = _flash()[0](q, k, v, 0.0, case.scale, False)
    assert out.shape == case.target.shape and out.is_contiguous()
    _same(out, case.target, "flash_attn_func")
    _same(ops.flash_attn_func(q, k, v, case.scale, False), case.target, "C ABI")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_tail_needle_bit_exact(dtype):
    case = C.TailCase(dtype)
    q, k, v = case.to(DEV)
    _same(_flash()[0](q, k, v, softmax_scale=case.scale, causal=False), case.target)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_poisoned_neighbour_heads_do_not_reach_head_one(dtype):
    case = C.poisoned(dtype)
    q, k, v = case.to(DEV)
    out = _flash()[0](q, k, v, causal=False)
    _same(out[:, :, 1].contiguous(), case.target[:, :, 1].contiguous())


@pytest.mark.parametrize("spec", C.VARLEN, ids=C.case_id)
def test_varlen_needles_bit_exact(spec):
    case = C.VarlenCase(spec)
    qkv, cu = case.qkv.to(DEV), case.cu_seqlens.to(DEV)
    out = _flash()[1](qkv, cu, case.max_seqlen, 0.0, softmax_scale=None, causal=False)
    assert out.shape == (case.rows, case.H, case.Dh) and out.is_contiguous()
    _same(out[:case.total], case.target, "flash_attn_varlen_qkvpacked_func")
    # the C ABI, into a buffer whose rows beyond cu_seqlens[-1] must keep their bits
    buf = torch.full((case.rows, case.H, case.Dh), SENTINEL, dtype=torch.int16, device=DEV).view(case.dtype)
    out2 = ops.attn_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, case.max_seqlen, out=buf)
    assert out2 is buf
    _same(buf[:case.total], case.target, "C ABI")
    assert (buf[case.total:].view(torch.int16) == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------------
# random inputs against float64, elementwise
# ------------------------------------------------------------------------------------------------------------------------
def _random(shape, dtype, g, mul=1.0, add=0.0):
    return (add + mul * torch.randn(*shape, generator=g, device=DEV)).to(dtype)


def _within(out, ref, Aw, qk, dtype, Sk, Dh):
    lim = O.bound(ref, Aw, qk, dtype, Sk, Dh, Dh ** -0.5)
    err = (out.double() - ref).abs()
    print(f"max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("B,H,Hkv,Sq,Sk", [(2, 4, 4, 200, 200), (1, 16, 16, 729, 729), (2, 2, 1, 100, 333)])
def test_dense_random_inputs_within_the_derived_bound(dtype, B, H, Hkv, Sq, Sk):
    """q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N (the distributions of tests/test_gpu_attention_prefill.py), q / k / v views of one qkv buffer."""
    g = torch.Generator(device=DEV).manual_seed(Sq * 31 + Sk)
    Dh, S = 72, max(Sq, Sk)
    qkv = torch.full((B, S, (H + 2 * Hkv) * Dh), float("nan"), dtype=dtype, device=DEV)
    q = qkv[:, :Sq, :H * Dh].view(B, Sq, H, Dh)
    k = qkv[:, :Sk, H * Dh:(H + Hkv) * Dh].view(B, Sk, Hkv, Dh)
    v = qkv[:, :Sk, (H + Hkv) * Dh:].view(B, Sk, Hkv, Dh)
    q.copy_(_random(q.shape, dtype, g, 1.5))
    k.copy_(_random(k.shape, dtype, g))
    v.copy_(_random(v.shape, dtype, g, 0.5, 1.0))
    out = _flash()[0](q, k, v, causal=False)
    assert torch.isfinite(out.float()).all()
    ref, Aw, qk = O.attention(q, k, v, None, False, stats=True)
    _within(out, ref, Aw, qk, dtype, Sk, Dh)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("Dh", [64, 72])
def test_varlen_random_inputs_within_the_derived_bound(dtype, Dh):
    lens, H = [1, 65, 0, 200, 729], 4
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    g = torch.Generator(device=DEV).manual_seed(Dh)
    qkv = torch.full((cu[-1] + 2, 3, H, Dh), float("nan"), dtype=dtype, device=DEV)
    qkv[:cu[-1], 0] = _random((cu[-1], H, Dh), dtype, g, 1.5)
    qkv[:cu[-1], 1] = _random((cu[-1], H, Dh), dtype, g)
    qkv[:cu[-1], 2] = _random((cu[-1], H, Dh), dtype, g, 0.5, 1.0)
    out = _flash()[1](qkv, torch.tensor(cu, dtype=torch.int32, device=DEV), max(lens))
    assert torch.isfinite(out[:cu[-1]].float()).all()
    ref, Aw, qk = C.varlen_oracle(qkv, cu, max(lens), stats=True)  # the oracle runs per sequence, on the GPU tensors
    for s, n in enumerate(lens):
        if n:
            b, e = cu[s], cu[s + 1]
            _within(out[b:e], ref[b:e], Aw[b:e], qk[b:e], dtype, n, Dh)  # the bound of a row takes its own sequence's key count


# ------------------------------------------------------------------------------------------------------------------------
# the two forms agree
# ------------------------------------------------------------------------------------------------------------------------
def _equal_length(B, S, H, Dh, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.cat([_random((B * S, 1, H, Dh), dtype, g, 1.5), _random((B * S, 1, H, Dh), dtype, g), _random((B * S, 1, H, Dh), dtype, g, 0.5, 1.0)], 1)
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=DEV)
    d = qkv.view(B, S, 3, H, Dh)
    return qkv, cu, (d[:, :, 0], d[:, :, 1], d[:, :, 2])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_equal_lengths_match_the_dense_prefill_kernel_at_head_dim_64(dtype):
    B, S, H, Dh = 3, 129, 4, 64
    qkv, cu, (q, k, v) = _equal_length(B, S, H, Dh, dtype, 7)
    f, fv = _flash()
    var = fv(qkv, cu, S).view(B, S, H, Dh)
    dense = f(q, k, v, causal=False)  # Dh = 64: csrc/awq_attn_prefill_cdna4.hip
    ref, Aw, qk = O.attention(q, k, v, None, False, stats=True)
    lim = O.bound(ref, Aw, qk, dtype, S, Dh, Dh ** -0.5)
    err = (var.double() - dense.double()).abs()
    assert not (err > lim).any(), float((err / lim).max())
    _within(var, ref, Aw, qk, dtype, S, Dh)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_equal_lengths_match_the_dense_form_bit_for_bit_at_head_dim_72(dtype):
    B, S, H, Dh = 3, 129, 4, 72
    qkv, cu, (q, k, v) = _equal_length(B, S, H, Dh, dtype, 9)
    f, fv = _flash()
    var = fv(qkv, cu, S)
    dense = f(q, k, v, causal=False)
    assert torch.equal(var.view(torch.int16).view(B, S, H, Dh), dense.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------
# every q tile, determinism, graph replay
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [32, 64, 128])
def test_every_q_tile_of_the_plan_is_bit_exact(rows_knob, rows):
    dense = C.dense_case(dict(name="tile", dtype=torch.float16, Dh=72, causal=False, fused=True, B=1, H=2, Hkv=1, Sq=729, Sk=729, mode="edges"))
    var = C.VarlenCase(dict(name="tile", dtype=torch.bfloat16, lens=[729, 100], H=2, Dh=64))
    rows_knob(rows)
    assert ops.attn_varlen_plan(1, 2, 72, 729) == (rows, 2 * -(-729 // rows)) == ops.attn_prefill_plan(1, 2, 1, 72, 729, 729, False)
    f, fv = _flash()
    q, k, v = dense.to(DEV)
    _same(f(q, k, v, causal=False), dense.target, rows)
    out = fv(var.qkv.to(DEV), var.cu_seqlens.to(DEV), var.max_seqlen)
    _same(out[:var.total], var.target, rows)


@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 72), (torch.bfloat16, 64)])
def test_same_call_twice_and_graph_replays_give_the_same_bits(dtype, Dh):
    lens, H = [300, 0, 729, 65], 8
    total = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(13)
    qkv = torch.cat([_random((total, 1, H, Dh), dtype, g, 1.5), _random((total, 1, H, Dh), dtype, g), _random((total, 1, H, Dh), dtype, g, 0.5, 1.0)], 1)
    cu = torch.tensor([0, 300, 300, 1029, 1094], dtype=torch.int32, device=DEV)
    fv = _flash()[1]
    a = fv(qkv, cu, 729)
    b = fv(qkv, cu, 729)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fv(qkv, cu, 729)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):  # a single kernel, no branches
        o = fv(qkv, cu, 729)
    for _ in range(3):
        o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), a.view(torch.int16))
