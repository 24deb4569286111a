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


# ------------------------------------------------------------------------------------------------------------------------
# long-context angles: positions up to 131071 put sincosf on its large-argument range reduction (angles of 1e5 rad at the first
# frequency); `check` and the oracle are the ones above, the angle is whatever fp32 value the caller hands over
# ------------------------------------------------------------------------------------------------------------------------
LONG_L = 131072
ROPE_BASES = [10000.0, 500000.0]


def _long_freqs(pos, d2, base):
    """[len(pos), 1, d2] fp32 angles pos * inv_freq, as the model builds them (flat index (s * B + b) * d2 + c with B = 1)"""
    inv = 1.0 / (base ** (torch.arange(0, d2, 2, device=DEV).float() / d2))
    f = torch.outer(pos.float(), inv)
    return torch.cat([f, f], -1).reshape(pos.numel(), 1, d2).contiguous()


def _long_positions(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pos = torch.randint(122880, LONG_L, (n,), generator=g, device=DEV)
    pos[0], pos[1] = LONG_L - 1, 65536
    return pos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("base", ROPE_BASES)
@pytest.mark.parametrize("d2", [64, 128])
def test_fused_rope_with_pos_at_long_context_angles(dtype, base, d2):
    """q and k as strided views of one fused qkv tensor, positions drawn from [122880, 131072) plus 131071 and 65536"""
    E = _engine()
    B, S, H, Hkv, Dh = 1, 66, 4, 2, 128
    g = torch.Generator(device=DEV).manual_seed(int(base) + d2)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * Dh, generator=g, device=DEV).to(dtype)
    fr = _long_freqs(_long_positions(S, d2), d2, base)
    assert float(fr.max()) > 1.2e5
    for lo, n in ((0, H), (H * Dh, Hkv)):
        x = qkv[:, :, lo:lo + n * Dh].view(B, S, n, Dh)
        assert not x.is_contiguous()
        for transpose in (False, True):
            out = E.fused_rope_with_pos_forward_func(x, fr, transpose)
            ref, mag = R.fused_rope_with_pos(x, fr)
            check(out, ref, mag, dtype)
            if d2 < Dh:
                assert torch.equal(out[..., d2:], x[..., d2:])
            out2 = ops.fused_rope_with_pos(x, fr, transpose)
            assert torch.equal(out2.contiguous().view(torch.int16), out.contiguous().view(torch.int16))


def _long_store_case(dtype, Dh, Hkv, base):
    H, S = 2 * Hkv, 33
    start = LONG_L - S
    g = torch.Generator(device=DEV).manual_seed(Dh + Hkv + int(base))
    W = (H + 2 * Hkv) * Dh
    wide = torch.full((1, S + 1, W + 24), float("nan"), dtype=dtype, device=DEV)  # a strided view, NaN around it
    qkv = wide[:, :S, 8:8 + W]
    qkv.copy_(torch.randn(1, S, W, generator=g, device=DEV))
    fr = _long_freqs(torch.arange(start, start + S, device=DEV), Dh, base)
    x = qkv.reshape(1, S, H + 2 * Hkv, Dh)
    xq, xk, xv = x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]
    return H, S, start, qkv, fr, xq, xk, xv


def _bits16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Dh,Hkv", [(64, 1), (128, 2)])
@pytest.mark.parametrize("layout", ["ft", "natural"])
def test_rope_kv_store_at_the_end_of_a_131072_token_cache(layout, Dh, Hkv, dtype):
    """rope_kv_store / rope_kv_store_natural with start_pos = 131072 - 33: the bits of the two rope calls plus the stores they replace (and the
    float64 bound on q and k), nothing written in the 64 positions before the window nor in the first 64 of a NaN-filled cache"""
    E = _engine()
    L = LONG_L
    for base in ROPE_BASES:
        H, S, start, qkv, fr, xq, xk, xv = _long_store_case(dtype, Dh, Hkv, base)
        q_want = E.fused_rope_with_pos_forward_func(xq, fr, True)
        k_rot = E.fused_rope_with_pos_forward_func(xk, fr, True)
        q_ref, q_mag = R.fused_rope_with_pos(xq, fr)
        k_ref, k_mag = R.fused_rope_with_pos(xk, fr)
        check(k_rot, k_ref, k_mag, dtype)
        nan = float("nan")
        if layout == "ft":
            kc = torch.full((1, Hkv, Dh // 8, L, 8), nan, dtype=dtype, device=DEV)
            vc = torch.full((1, Hkv, L, Dh), nan, dtype=dtype, device=DEV)
            fns = (ops.rope_kv_store, E.rope_kv_store)
        else:
            kc = torch.full((1, L, Hkv, Dh), nan, dtype=dtype, device=DEV)
            vc = torch.full((1, L, Hkv, Dh), nan, dtype=dtype, device=DEV)
            fns = (ops.rope_kv_store_natural, E.rope_kv_store_natural)
        for fn in fns:
            q_out = fn(qkv, fr, kc, vc, start, H, Hkv)
            torch.cuda.synchronize()
            assert q_out.shape == (1, S, H, Dh) and torch.equal(_bits16(q_out), _bits16(q_want))
            check(q_out, q_ref, q_mag, dtype)
            if layout == "ft":
                k_win = kc[:, :, :, start:].permute(0, 3, 1, 2, 4).reshape(1, S, Hkv, Dh)
                v_win = vc[:, :, start:].transpose(1, 2)
                untouched = (kc[:, :, :, start - 64:start], kc[:, :, :, :64], vc[:, :, start - 64:start], vc[:, :, :64])
            else:
                k_win, v_win = kc[:, start:], vc[:, start:]
                untouched = (kc[:, start - 64:start], kc[:, :64], vc[:, start - 64:start], vc[:, :64])
            assert torch.equal(_bits16(k_win), _bits16(k_rot)) and torch.equal(_bits16(v_win), _bits16(xv))
            assert all(bool(torch.isnan(u).all()) for u in untouched), "written outside [start_pos, start_pos + S)"
            if layout == "ft":  # (poison the window again for the second entry point)
                kc[:, :, :, start:] = nan
                vc[:, :, start:] = nan
            else:
                kc[:, start:] = nan
                vc[:, start:] = nan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Dh,Hkv", [(64, 1), (128, 2)])
def test_rope_kv_store_natural_fp8_at_the_end_of_a_131072_token_cache(Dh, Hkv, dtype):
    """the fp8 store at start_pos = 131072 - 33: q bit for bit, codes and scales against tests/kv8_oracle.py's quantiser of the rotated K and of V,
    the sentinel left in the 64 positions before the window and in the first 64"""
    import numpy as np
    from tests import kv8_oracle as K8
    E = _engine()
    L = LONG_L
    dt = "f16" if dtype == torch.float16 else "bf16"
    code_s, scale_s = 0xA5, -7.25

    def np_of(t):
        return K8.from_bits(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dt)

    for base in ROPE_BASES:
        H, S, start, qkv, fr, xq, xk, xv = _long_store_case(dtype, Dh, Hkv, base)
        q_want = E.fused_rope_with_pos_forward_func(xq, fr, True)
        k_rot = E.fused_rope_with_pos_forward_func(xk, fr, True)
        want_kc, want_ks = K8.quant(np_of(k_rot))
        want_vc, want_vs = K8.quant(np_of(xv))
        for fn, cache_dtype in ((ops.rope_kv_store_natural_fp8, torch.float8_e4m3fn), (E.rope_kv_store_natural_fp8, torch.uint8)):
            kc = torch.full((1, L, Hkv, Dh), code_s, dtype=torch.uint8, device=DEV).view(cache_dtype)
            vc = torch.full((1, L, Hkv, Dh), code_s, dtype=torch.uint8, device=DEV).view(cache_dtype)
            ks = torch.full((1, L, Hkv), scale_s, device=DEV)
            vs = torch.full((1, L, Hkv), scale_s, device=DEV)
            q_out = fn(qkv, fr, kc, vc, ks, vs, start, H, Hkv)
            torch.cuda.synchronize()
            assert torch.equal(_bits16(q_out), _bits16(q_want))
            for name, cache, scale, wc, ws in (("k", kc, ks, want_kc, want_ks), ("v", vc, vs, want_vc, want_vs)):
                c8 = cache.view(torch.uint8)
                assert np.array_equal(c8[:, start:].cpu().numpy(), wc), name + " codes"
                assert np.array_equal(scale[:, start:].cpu().numpy().view(np.uint32), ws.view(np.uint32)), name + " scales"
                for sl in (slice(start - 64, start), slice(0, 64)):
                    assert bool((c8[:, sl] == code_s).all()) and bool((scale[:, sl] == scale_s).all()), name + " written outside the window"
