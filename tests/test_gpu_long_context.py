"""The long-context mode on the MI355X: rope_kv_store_natural (csrc/awq_attn_chunk_cdna4.hip) against the two rope calls and the two
slice stores it replaces, and QuantLlamaAttentionFused(kv_layout="natural") against a restatement of tinychat's long_forward
(tinychat/modules/fused_attn.py:505-546) written here from the engine's separate calls.  The reference tree is not read."""
import math
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_oracle as O
from tests import attn_splitkv_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


def split_qkv(qkv, H, Hkv):
    """fused_attn.py:514-525: views of the fused projection, [B, S, heads, Dh] each."""
    B, S, W = qkv.shape
    Dh = W // (H + 2 * Hkv)
    x = qkv.view(B, S, H + 2 * Hkv, Dh) if qkv.is_contiguous() else qkv.reshape(B, S, H + 2 * Hkv, Dh)
    return x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]


def _sentinel(shape, dtype, mul):
    n = math.prod(shape)
    return ((torch.arange(n, device=DEV) * mul + 12345) % 30011).to(torch.int16).view(dtype).reshape(shape).clone()  # finite, positive


# ------------------------------------------------------------------------------------------------------------------------
# rope_kv_store_natural: the bits of rope x 2 plus the slice stores, and nothing written outside the window
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Dh,half_rot", [(64, False), (128, False), (128, True)])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 33])
def test_rope_kv_store_natural_bits_and_footprint(S, B, Dh, half_rot, dtype):
    E = _engine()
    H, Hkv, L, Bc = 4, 2, 61, 3
    rot = Dh // 2 if half_rot else Dh
    W = (H + 2 * Hkv) * Dh
    for start in (0, 17):
        g = torch.Generator(device=DEV).manual_seed(S * 7 + start + B)
        if start == 0:
            qkv = torch.randn(B, S, W, generator=g, device=DEV).to(dtype)
        else:  # a strided slice of a wider buffer (NaN around it)
            wide = torch.full((B, S + 1, W + 24), float("nan"), dtype=dtype, device=DEV)
            qkv = wide[:, :S, 8:8 + W]
            qkv.copy_(torch.randn(B, S, W, generator=g, device=DEV))
        freqs = (50.0 * torch.randn(S, B, rot, generator=g, device=DEV)).contiguous()  # read flat at (s * B + b) * rot + c
        kc0, vc0 = _sentinel((Bc, L, Hkv, Dh), dtype, 7), _sentinel((Bc, L, Hkv, Dh), dtype, 13)
        # the composition it replaces (long_forward): two rope calls, two slice stores
        xq, xk, xv = split_qkv(qkv, H, Hkv)
        q_want = E.fused_rope_with_pos_forward_func(xq, freqs, True)
        k_rot = E.fused_rope_with_pos_forward_func(xk, freqs, True)
        kc_want, vc_want = kc0.clone(), vc0.clone()
        vc_want[:B, start:start + S] = xv
        kc_want[:B, start:start + S] = k_rot
        for fn in (ops.rope_kv_store_natural, E.rope_kv_store_natural):
            kc, vc = kc0.clone(), vc0.clone()
            q_out = fn(qkv, freqs, kc, vc, start, H, Hkv)
            torch.cuda.synchronize()
            assert q_out.shape == (B, S, H, Dh) and q_out.is_contiguous()
            assert torch.equal(bits(q_out), bits(q_want))
            assert torch.equal(bits(kc), bits(kc_want)) and torch.equal(bits(vc), bits(vc_want))
            # the footprint, against the sentinel itself
            keep = torch.ones(L, dtype=torch.bool, device=DEV)
            keep[start:start + S] = False
            assert torch.equal(bits(kc[:, keep]), bits(kc0[:, keep])) and torch.equal(bits(vc[:, keep]), bits(vc0[:, keep]))
            assert torch.equal(bits(kc[B:]), bits(kc0[B:])) and torch.equal(bits(vc[B:]), bits(vc0[B:]))
            assert not torch.equal(bits(kc[:B, start:start + S]), bits(kc0[:B, start:start + S]))


def test_rope_kv_store_natural_refuses_what_does_not_fit():
    E = _engine()
    B, S, H, Hkv, Dh, L = 2, 8, 4, 2, 64, 16
    qkv = torch.zeros(B, S, (H + 2 * Hkv) * Dh, dtype=torch.float16, device=DEV)
    fr = torch.zeros(S, B, Dh, device=DEV)
    kc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float16, device=DEV)
    vc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="do not fit"):
        E.rope_kv_store_natural(qkv, fr, kc, vc, 9, H, Hkv)
    with pytest.raises(_capi.AwqNativeError):
        ops.rope_kv_store_natural(qkv, fr, kc, vc, 9, H, Hkv)
    with pytest.raises(RuntimeError, match="cache batch"):
        E.rope_kv_store_natural(qkv, fr, kc[:1], vc[:1], 0, H, Hkv)
    with pytest.raises(RuntimeError, match="dtype"):
        E.rope_kv_store_natural(qkv, fr, kc.bfloat16(), vc.bfloat16(), 0, H, Hkv)
    with pytest.raises(RuntimeError, match="one shape"):
        E.rope_kv_store_natural(qkv, fr, kc, vc[:, :8].contiguous(), 0, H, Hkv)
    assert not kc.any() and not vc.any()


# ------------------------------------------------------------------------------------------------------------------------
# the module in natural mode, tiny: prompt 40, chunk 9, three decode steps; one decode step over a long history
# ------------------------------------------------------------------------------------------------------------------------
FLOW = dict(B=1, H=4, Hkv=2, Dh=128, L=8200, steps=(40, 9, 1, 1, 1))  # hidden 512


def _freqs(start, n, Dh, base=10000.0):
    inv = 1.0 / (base ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(start, start + n, device=DEV).float(), inv)
    return torch.cat([f, f], -1)[None].contiguous()  # [1, n, Dh]: one angle per column, rotate-half layout


def _inputs(dtype, steps, seed=3):
    """qkv tensors with the distributions the attention bounds are meant for (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N)."""
    B, H, Hkv, Dh = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"]
    mul = torch.cat([torch.full((H * Dh,), 1.5), torch.ones(Hkv * Dh), torch.full((Hkv * Dh,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + Hkv) * Dh), torch.ones(Hkv * Dh)]).to(DEV)
    gg = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.randn(B, S, (H + 2 * Hkv) * Dh, generator=gg, device=DEV) * mul + add).to(dtype) for S in steps]


def _module(**kw):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    H, Hkv, Dh = FLOW["H"], FLOW["Hkv"], FLOW["Dh"]
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=Hkv, hidden_size=H * Dh, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=FLOW["L"])
    # the projections are stand-ins: x already is the qkv tensor and the output is returned as it is, so only the attention is under test
    return QuantLlamaAttentionFused(H * Dh, H, kw.pop("L", FLOW["L"]), torch.nn.Identity(), torch.nn.Identity(), DEV, args, **kw)


def long_forward(E, qkv, start_pos, freqs, cache_k, cache_v, H, Hkv):
    """fused_attn.py:505-546 from the engine's separate calls: rope x 2, the slice stores, the one-pass attention on the cached history."""
    B, S, _ = qkv.shape
    xq, xk, xv = split_qkv(qkv, H, Hkv)
    xq = E.fused_rope_with_pos_forward_func(xq, freqs, True)
    xk = E.fused_rope_with_pos_forward_func(xk, freqs, True)
    cache_v[:B, start_pos:start_pos + S] = xv
    cache_k[:B, start_pos:start_pos + S] = xk
    out = E.attn_prefill(xq, cache_k[:B, :start_pos + S], cache_v[:B, :start_pos + S], xq.shape[-1] ** -0.5, True)
    return out.view(B, S, -1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_in_natural_mode_is_long_forward_bit_for_bit(dtype):
    E = _engine()
    B, H, Hkv, Dh, L = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"], FLOW["L"]
    xs = _inputs(dtype, FLOW["steps"])
    m = _module(kv_layout="natural")
    assert tuple(m.cache_k.shape) == tuple(m.cache_v.shape) == (1, L, Hkv, Dh) and m.kv_layout == "natural"
    ck = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
    cv = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
    pos = 0
    for x in xs:
        S = x.shape[1]
        fr = _freqs(pos, S, Dh)
        ours = m(x, pos, fr, None, chunk_prefilling=(S > 1 and pos > 0))
        want = long_forward(E, x, pos, fr, ck, cv, H, Hkv)
        torch.cuda.synchronize()
        assert ours.shape == (B, S, H * Dh)
        assert torch.equal(bits(ours), bits(want)), (pos, S, int((bits(ours) != bits(want)).sum()))  # Sk < 2048: the same kernel, the same bits
        pos += S
    assert m.cache_k.dtype == dtype and pos == 52
    assert torch.equal(bits(m.cache_k), bits(ck)) and torch.equal(bits(m.cache_v), bits(cv))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_decode_step_over_a_long_history_takes_the_split_kernels(dtype):
    E = _engine()
    B, H, Hkv, Dh, L = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"], FLOW["L"]
    pos = 4100
    m = _module(kv_layout="natural")
    g = torch.Generator(device=DEV).manual_seed(5)
    hist_k = torch.randn(B, pos, Hkv, Dh, generator=g, device=DEV).to(dtype)
    hist_v = (1 + 0.5 * torch.randn(B, pos, Hkv, Dh, generator=g, device=DEV)).to(dtype)
    m.cache_k = m.cache_k.to(dtype)
    m.cache_v = m.cache_v.to(dtype)
    m.cache_k[:, :pos], m.cache_v[:, :pos] = hist_k, hist_v  # the history, written directly
    x, = _inputs(dtype, (1,), seed=9)
    fr = _freqs(pos, 1, Dh)
    splits = ops.attn_splitkv_plan(B, H, Hkv, Dh, 1, pos + 1, True)[0]
    assert splits > 1
    out = m(x, pos, fr, None)
    torch.cuda.synchronize()
    # the float64 oracle on the rotated q and the cache the module left behind
    xq, xk, xv = split_qkv(x, H, Hkv)
    q = E.fused_rope_with_pos_forward_func(xq, fr, True)
    assert torch.equal(bits(m.cache_k[:, pos:pos + 1]), bits(E.fused_rope_with_pos_forward_func(xk, fr, True)))
    assert torch.equal(bits(m.cache_v[:, pos:pos + 1]), bits(xv)) and torch.equal(bits(m.cache_k[:, :pos]), bits(hist_k))
    ref, Aw, qk = O.attention(q, m.cache_k[:B, :pos + 1], m.cache_v[:B, :pos + 1], None, True, stats=True)
    lim = S.bound(ref, Aw, qk, dtype, pos + 1, Dh, Dh ** -0.5, splits)
    err = (out.view(B, 1, H, Dh).double() - ref).abs()
    print(f"max err / bound = {float((err / lim).max()):.3f}")
    assert torch.isfinite(out.float()).all() and not (err > lim).any(), float((err / lim).max())
    assert torch.equal(bits(out.view(B, 1, H, Dh)), bits(ops.attn_splitkv(q, m.cache_k[:B, :pos + 1], m.cache_v[:B, :pos + 1], None, True)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ft_mode_is_unchanged_by_the_keyword(dtype):
    xs = _inputs(dtype, (40, 9, 1))
    a, b = _module(L=256), _module(L=256, kv_layout="ft")
    assert a.kv_layout == b.kv_layout == "ft" and a.cache_k.shape == b.cache_k.shape == (1, FLOW["Hkv"], FLOW["Dh"] // 8, 256, 8)
    pos = 0
    for x in xs:
        S = x.shape[1]
        fr = _freqs(pos, S, FLOW["Dh"]) if S > 1 else None
        oa, ob = a(x, pos, fr, None, chunk_prefilling=pos > 0), b(x, pos, fr, None, chunk_prefilling=pos > 0)
        assert torch.equal(bits(oa), bits(ob))
        pos += S
    assert torch.equal(bits(a.cache_k), bits(b.cache_k)) and torch.equal(bits(a.cache_v), bits(b.cache_v))
    with pytest.raises(ValueError, match="kv_layout"):
        _module(kv_layout="paged")
