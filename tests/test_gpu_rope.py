"""The rotary-embedding exports on the MI355X (csrc/awq_attn_prefill_cdna4.hip) against their float64 restatements (tests/rope_oracle.py):
elementwise |out - ref| <= 1/2 ulp_T(ref) + 4 * 2^-23 * (|x| + |x_rot|) -- one rounding to T plus fp32 evaluation (device sincosf is
within 2 ulp of fp32; for rotary_embedding_neox cos / sin come from the cache and only fp32 rounding remains)."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from tests import attn_oracle as A
from tests import rope_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def check(out, ref, mag, dtype):
    assert torch.isfinite(out.float()).all()
    lim = 0.5 * A.ulp(ref, dtype) + 4 * 2.0 ** -23 * mag
    err = (out.double() - ref).abs()
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), float((err / lim).max()))


def _freqs(n_rows, n_cols, d2, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d2, 2, device=DEV).float() / d2))
    t = torch.randint(0, 8192, (n_rows * n_cols,), generator=g, device=DEV).float()
    f = torch.outer(t, inv)
    return torch.cat([f, f], -1).reshape(n_rows, n_cols, d2).contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n0,n1,h,d,d2", [(1, 300, 8, 128, 128), (2, 37, 4, 128, 128), (1, 65, 3, 64, 64), (3, 5, 2, 128, 64), (1, 1, 32, 128, 128)])
def test_fused_rope_with_pos(dtype, transpose, n0, n1, h, d, d2):
    E = _engine()
    g = torch.Generator(device=DEV).manual_seed(n1 + d2)
    x = torch.randn(n0, n1, h, d, generator=g, device=DEV).to(dtype)
    fr = _freqs(n0, n1, d2, seed=n0 + n1)  # tinychat's [bsz, seqlen, d2]; read by the flat index whatever its shape says
    out = E.fused_rope_with_pos_forward_func(x, fr, transpose)
    assert out.shape == x.shape and out.dtype == dtype
    want = torch.empty(n1, n0, h, d).transpose(0, 1).stride() if transpose else torch.empty(n0, n1, h, d).stride()
    assert out.stride() == want
    ref, mag = R.fused_rope_with_pos(x, fr)
    check(out, ref, mag, dtype)
    if d2 < d:
        assert torch.equal(out[..., d2:], x[..., d2:])
    out2 = ops.fused_rope_with_pos(x, fr, transpose)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and out2.stride() == want


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rope_with_pos_flat_index_at_two_batch_rows(dtype):
    """(i0, i1) reads row i1 * n0 + i0 of the angles: with freqs of shape [n0, n1, d2] that is NOT freqs[i0, i1] when n0 = 2."""
    E = _engine()
    n0, n1, h, d = 2, 6, 2, 128
    x = torch.randn(n0, n1, h, d, device=DEV).to(dtype)
    fr = _freqs(n0, n1, d, seed=9)
    out = E.fused_rope_with_pos_forward_func(x, fr, False)
    ref, mag = R.fused_rope_with_pos(x, fr)
    check(out, ref, mag, dtype)
    naive, _ = R.fused_rope_with_pos(x, fr.reshape(n0, n1, d).transpose(0, 1).contiguous())  # what indexing freqs[i0, i1] would give
    assert float((out.double() - naive).abs().max()) > 0.1


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rope_with_pos_on_strided_views(dtype):
    """q and k as views of one fused qkv tensor (fused_attn.py:242-246), and a view whose last stride is not 1."""
    E = _engine()
    B, S, H, Hkv, Dh = 1, 130, 8, 2, 128
    qkv = torch.randn(B, S, (H + 2 * Hkv) * Dh, device=DEV).to(dtype)
    fr = _freqs(B, S, Dh, seed=4)
    for lo, n in ((0, H), (H * Dh, Hkv)):
        x = qkv[:, :, lo:lo + n * Dh].view(B, S, n, Dh)
        assert not x.is_contiguous()
        out = E.fused_rope_with_pos_forward_func(x, fr, True)
        ref, mag = R.fused_rope_with_pos(x, fr)
        check(out, ref, mag, dtype)
    xt = torch.randn(B, S, Dh, 4, device=DEV).to(dtype).transpose(2, 3)  # [B, S, 4, Dh] with stride(3) = 4
    out = E.fused_rope_with_pos_forward_func(xt, fr, False)
    ref, mag = R.fused_rope_with_pos(xt, fr)
    check(out, ref, mag, dtype)


def test_fused_rope_with_pos_refuses_float32():
    E = _engine()
    with pytest.raises(RuntimeError, match="float32"):
        E.fused_rope_with_pos_forward_func(torch.zeros(1, 4, 2, 64, device=DEV), torch.zeros(1, 4, 64, device=DEV), True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,heads,hs,rot", [(50, 4, 128, 128), (300, 32, 128, 128), (7, 3, 64, 32), (1, 8, 128, 64)])
def test_rotary_embedding_neox_in_place(dtype, T, heads, hs, rot):
    E = _engine()
    mp = 2048
    g = torch.Generator(device=DEV).manual_seed(T + rot)
    # query and key live inside NaN-guarded allocations: nothing outside them may be read into the result or written
    pad = 64
    qb = torch.full((pad + T * heads * hs + pad,), float("nan"), dtype=dtype, device=DEV)
    kb = torch.full((pad + T * heads * hs + pad,), float("nan"), dtype=dtype, device=DEV)
    q = qb[pad:pad + T * heads * hs].view(1, T, heads, hs)
    k = kb[pad:pad + T * heads * hs].view(1, T, heads, hs)
    q.copy_(torch.randn(1, T, heads, hs, generator=g, device=DEV))
    k.copy_(torch.randn(1, T, heads, hs, generator=g, device=DEV))
    pos = torch.randint(0, mp, (1, T), generator=g, device=DEV)
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, device=DEV).double() / rot))
    ang = torch.outer(torch.arange(mp, device=DEV).double(), inv)
    cache = torch.cat([ang.cos(), ang.sin()], -1).to(dtype)
    rq, mq = R.rotary_embedding_neox(pos, q, hs, cache)
    rk, mk = R.rotary_embedding_neox(pos, k, hs, cache)
    q0 = q.clone()
    assert E.rotary_embedding_neox(pos, q, k, hs, cache) is None
    check(q, rq, mq, dtype)
    check(k, rk, mk, dtype)
    if rot < hs:
        assert torch.equal(q[..., rot:], q0[..., rot:])
    for buf in (qb, kb):
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all()
    # the ctypes path gives the same bits
    q2 = q0.clone()
    k2 = k.clone()
    ops.rotary_embedding_neox(pos, q2, k2, hs, cache)
    assert torch.equal(q2.view(torch.int16), q.view(torch.int16))
