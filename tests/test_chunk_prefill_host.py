"""Chunk prefill on the FT KV cache without a GPU: the exports of awq_rope_kv_store / awq_attn_prefill_ftcache, every argument code of
the two C entries, the bindings' refusals, the module layer (llm_awq_amd/fused_attn.py) on the CPU, and the float64 restatement of
rope_kv_store (tests/chunk_prefill_oracle.py) against the reference's own stores (tests/test_gpu_chunk_prefill.py compares the
kernel with that restatement)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.qmodule import WQLinear, pack_intweight, unpack_intweight
from tests import chunk_prefill_oracle as CP
from tests import rope_oracle as R

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL = -3, -4, -5, -6


# ------------------------------------------------------------------------------------------------------------------------
# 1. symbols and bindings
# ------------------------------------------------------------------------------------------------------------------------
def test_library_and_engine_export_the_chunk_prefill_surface():
    L = _capi.lib()
    for name in ("awq_rope_kv_store", "awq_attn_prefill_ftcache"):
        assert hasattr(L, name), name
        assert name in _capi.SIGNATURES, name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]

    assert params(eng.rope_kv_store) == ["qkv", "freqs", "k_cache", "v_cache", "start_pos", "nheads", "nheads_kv"]
    assert params(eng.attn_prefill_ftcache) == ["q", "k_cache", "v_cache", "kv_start", "seqlen_k", "softmax_scale", "causal"]
    assert callable(ops.rope_kv_store) and callable(ops.attn_prefill_ftcache)
    assert llm_awq_amd.make_quant_attn is not None and llm_awq_amd.QuantLlamaAttentionFusedFlash is llm_awq_amd.QuantLlamaAttentionFused
    for name in ("QuantLlamaAttentionFused", "QuantLlamaAttentionFusedFlash", "make_quant_attn"):
        assert name in llm_awq_amd.__all__


# ------------------------------------------------------------------------------------------------------------------------
# 2. argument codes, no GPU call
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _store(p, **kw):
    a = dict(qkv=p, freqs=p, q_out=p, k_cache=p, v_cache=p, B=1, Bc=2, S=16, H=8, Hkv=2, Dh=128, rot=128, lmax=64, start=3, bs=16 * 1536,
             rs=1536, dtype=0)
    a.update(kw)
    return _capi.lib().awq_rope_kv_store(a["qkv"], a["freqs"], a["q_out"], a["k_cache"], a["v_cache"], a["B"], a["Bc"], a["S"], a["H"], a["Hkv"],
                                         a["Dh"], a["rot"], a["lmax"], a["start"], a["bs"], a["rs"], a["dtype"], None)


def _attn(p, **kw):
    a = dict(q=p, k_cache=p, v_cache=p, out=p, B=1, Bc=2, Sq=16, kv_start=3, Sk=20, H=8, Hkv=2, Dh=128, lmax=64, qbs=16 * 1024, qrs=1024,
             scale=0.1, causal=1, dtype=0)
    a.update(kw)
    return _capi.lib().awq_attn_prefill_ftcache(a["q"], a["k_cache"], a["v_cache"], a["out"], a["B"], a["Bc"], a["Sq"], a["kv_start"], a["Sk"],
                                                a["H"], a["Hkv"], a["Dh"], a["lmax"], a["qbs"], a["qrs"], a["scale"], a["causal"], a["dtype"], None)


def test_rope_kv_store_validation_returns_codes_without_launch():
    buf, p = _p16()
    for bad in (dict(Dh=72, rs=8 * 12 * 72), dict(Dh=96), dict(Dh=32), dict(Dh=256, rs=4096), dict(B=3), dict(B=0), dict(S=0), dict(H=0),
                dict(Hkv=0), dict(start=-1), dict(start=49), dict(S=62), dict(lmax=0), dict(rot=24), dict(rot=120), dict(rot=0), dict(rot=144),
                dict(rot=136), dict(rs=1528), dict(bs=-8)):
        assert _store(p, **bad) == AWQ_ERR_SHAPE, bad
    # the last position that fits is accepted as far as the shape check goes: what follows is the alignment check
    assert _store(p, start=48, qkv=p + 2) == AWQ_ERR_ALIGN
    assert _store(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "freqs", "q_out", "k_cache", "v_cache"):
        assert _store(p, **{name: None}) == AWQ_ERR_NULL, name
        assert _store(p, **{name: p + 4}) == AWQ_ERR_ALIGN, name
    assert _store(p, rs=1540) == AWQ_ERR_ALIGN and _store(p, bs=16 * 1536 + 4) == AWQ_ERR_ALIGN


def test_attn_prefill_ftcache_validation_returns_codes_without_launch():
    buf, p = _p16()
    for bad in (dict(Dh=72, causal=0), dict(Dh=72), dict(Dh=96), dict(Dh=32), dict(B=3), dict(B=0), dict(Sq=0), dict(Sk=0), dict(H=0), dict(Hkv=0),
                dict(H=6, Hkv=4), dict(kv_start=-1), dict(kv_start=45), dict(Sk=62), dict(lmax=0), dict(Sq=21), dict(qrs=1016), dict(qbs=-8)):
        assert _attn(p, **bad) == AWQ_ERR_SHAPE, bad
    assert _attn(p, kv_start=44, q=p + 2) == AWQ_ERR_ALIGN    # kv_start + Sk == lmax passes the shape check
    assert _attn(p, Sq=21, causal=0, q=p + 2) == AWQ_ERR_ALIGN  # Sq > Sk is refused only under the causal mask
    assert _attn(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k_cache", "v_cache", "out"):
        assert _attn(p, **{name: None}) == AWQ_ERR_NULL, name
        assert _attn(p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _attn(p, qrs=1028) == AWQ_ERR_ALIGN and _attn(p, qbs=16 * 1024 + 4) == AWQ_ERR_ALIGN


def test_bindings_refuse_cpu_tensors_and_float32():
    eng = llm_awq_amd.load_engine()
    B, S, H, Hkv, Dh, L = 1, 4, 2, 1, 64, 16
    qkv = torch.zeros(B, S, (H + 2 * Hkv) * Dh, dtype=torch.float16)
    q = torch.zeros(B, S, H, Dh, dtype=torch.float16)
    fr = torch.zeros(B, S, Dh)
    kc = torch.zeros(B, Hkv, Dh // 8, L, 8, dtype=torch.float16)
    vc = torch.zeros(B, Hkv, L, Dh, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.rope_kv_store(qkv, fr, kc, vc, 0, H, Hkv)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.attn_prefill_ftcache(q, kc, vc, 0, S, 0.125, True)
    with pytest.raises(RuntimeError, match="float32"):
        eng.rope_kv_store(qkv.float(), fr, kc.float(), vc.float(), 0, H, Hkv)
    with pytest.raises(RuntimeError, match="float32"):
        eng.attn_prefill_ftcache(q.float(), kc.float(), vc.float(), 0, S, 0.125, True)
    with pytest.raises(_capi.AwqNativeError):
        ops.rope_kv_store(qkv, fr, kc, vc, 0, H, Hkv)
    with pytest.raises(_capi.AwqNativeError):
        ops.attn_prefill_ftcache(q, kc, vc, 0, S)
    assert not torch.cuda.is_initialized()


# ------------------------------------------------------------------------------------------------------------------------
# 3. the module layer on the CPU
# ------------------------------------------------------------------------------------------------------------------------
def _args(H, Hkv, Dh, rope_scaling=None):
    return SimpleNamespace(num_attention_heads=H, num_key_value_heads=Hkv, hidden_size=H * Dh, rope_theta=500000.0, rope_scaling=rope_scaling,
                           max_position_embeddings=4096)


@pytest.mark.parametrize("H,Hkv,Dh", [(8, 8, 128), (32, 8, 128), (12, 2, 64)])
def test_fused_attn_constructor_attributes_and_cache_shapes(H, Hkv, Dh):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused, QuantLlamaAttentionFusedFlash
    assert QuantLlamaAttentionFusedFlash is QuantLlamaAttentionFused
    qkv, o = torch.nn.Identity(), torch.nn.Identity()
    m = QuantLlamaAttentionFused(H * Dh, H, 96, qkv, o, "cpu", _args(H, Hkv, Dh), max_batch_size=3)
    assert (m.n_local_heads, m.num_heads, m.num_key_value_heads, m.num_key_value_groups, m.head_dim, m.hidden_size) == (H, H, Hkv, H // Hkv, Dh, H * Dh)
    assert m.kv_max_seq_len == 96 and m.rope_theta == 500000.0 and m.qkv_proj is qkv and m.o_proj is o
    assert m.cache_k.shape == (3, Hkv, Dh // 8, 96, 8) and m.cache_v.shape == (3, Hkv, 96, Dh)
    assert m.cache_k.dtype == torch.float16 and m.cache_v.dtype == torch.float16  # until the first forward, as the reference's .half()
    assert not m.cache_k.any() and not m.cache_v.any()
    assert QuantLlamaAttentionFused(H * Dh, H, 8, qkv, o, "cpu", _args(H, Hkv, Dh)).cache_v.shape[0] == 1
    assert "long" in (llm_awq_amd.fused_attn.__doc__ or "")  # the natural-layout long-context variant is named as out of scope


def test_fused_attn_rope_scaling_spellings_and_head_dim():
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    mk = lambda rs: QuantLlamaAttentionFused(256, 2, 8, torch.nn.Identity(), torch.nn.Identity(), "cpu", _args(2, 1, 128, rs)).rope_scaling
    assert mk(None) == 1.0 and mk({"factor": 4.0, "type": "linear"}) == 4.0 and mk({"type": "dynamic"}) == 1.0 and mk(2.5) == 2.5
    with pytest.raises(ValueError, match="head dim"):
        QuantLlamaAttentionFused(192, 2, 8, torch.nn.Identity(), torch.nn.Identity(), "cpu", _args(2, 1, 96))


def _proj(n, k, bias, seed, group=128):
    g = torch.Generator().manual_seed(seed)
    m = WQLinear(4, group, k, n, bias, "cpu")
    m.qweight = pack_intweight(torch.randint(0, 16, (n, k), generator=g, dtype=torch.int32))
    gpad, groups = m.scales.shape[0], k // group
    m.scales = torch.zeros(gpad, n, dtype=torch.float16)
    m.scales[:groups] = (torch.rand(groups, n, generator=g) * 0.02 + 0.005).half()
    m.scaled_zeros = torch.zeros(gpad, n, dtype=torch.float16)
    m.scaled_zeros[:groups] = (-(torch.rand(groups, n, generator=g) * 0.1)).half()
    if bias:
        m.bias = torch.randn(n, generator=g).half()
    return m


def _dequant(m):
    """[N, K] float32: q * scale + scaled_zero, the stored nibbles unsigned (the checkpoint contract)."""
    q = unpack_intweight(m.qweight).float()
    gi = torch.arange(m.in_features) // m.group_size
    return q * m.scales.float()[gi].t() + m.scaled_zeros.float()[gi].t()


class _Attn(torch.nn.Module):
    def __init__(self, H, Hkv, Dh, bias, seed=0):
        super().__init__()
        self.q_proj = _proj(H * Dh, H * Dh, bias, seed + 1)
        self.k_proj = _proj(Hkv * Dh, H * Dh, bias, seed + 2)
        self.v_proj = _proj(Hkv * Dh, H * Dh, bias, seed + 3)
        self.o_proj = _proj(H * Dh, H * Dh, False, seed + 4)
        self.args = _args(H, Hkv, Dh)
        self.kv_max_seq_len = 32


class _Block(torch.nn.Module):
    def __init__(self, bias):
        super().__init__()
        self.self_attn = _Attn(4, 2, 64, bias)
        self.mlp = torch.nn.Linear(8, 8)


@pytest.mark.parametrize("bias", [False, True])
def test_make_quant_attn_concatenates_the_projections(bias):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused, make_quant_attn
    model = torch.nn.Sequential(_Block(bias), _Block(bias))
    old = [blk.self_attn for blk in model]
    out = make_quant_attn(model, "cpu")
    assert out is model
    for blk, m in zip(model, old):
        a = blk.self_attn
        assert isinstance(a, QuantLlamaAttentionFused) and a.o_proj is m.o_proj and isinstance(blk.mlp, torch.nn.Linear)
        assert a.kv_max_seq_len == 32 and a.cache_k.shape == (1, 2, 8, 32, 8) and a.cache_v.shape == (1, 2, 32, 64)
        f = a.qkv_proj
        n = 4 * 64 + 2 * 2 * 64
        assert isinstance(f, WQLinear) and f.layout == "v2" and (f.in_features, f.out_features, f.w_bit, f.group_size) == (256, n, 4, 128)
        assert f.qweight.shape == (n // 4, 256) and f.qweight.dtype == torch.int16
        assert f.scales.shape == (m.q_proj.scales.shape[0], n) and f.scaled_zeros.shape == f.scales.shape
        assert f.scales.is_contiguous() and f.scaled_zeros.is_contiguous() and f.split_k_iters == m.q_proj.split_k_iters
        want = torch.cat([_dequant(m.q_proj), _dequant(m.k_proj), _dequant(m.v_proj)], 0)
        assert torch.equal(_dequant(f), want)
        assert torch.equal(unpack_intweight(f.qweight), torch.cat([unpack_intweight(p.qweight) for p in (m.q_proj, m.k_proj, m.v_proj)], 0))
        if bias:
            assert torch.equal(f.bias, torch.cat([m.q_proj.bias, m.k_proj.bias, m.v_proj.bias]))
        else:
            assert f.bias is None


def test_make_quant_attn_refuses_a_converted_projection():
    from llm_awq_amd.fused_attn import make_quant_attn
    model = torch.nn.Sequential(_Block(False))
    model[0].self_attn.k_proj.layout = "cdna4"  # what to_cdna4() leaves behind: the same buffers, qweight permuted
    with pytest.raises(RuntimeError, match="cdna4_restore"):
        make_quant_attn(model, "cpu")
    assert isinstance(model[0].self_attn, _Attn)  # nothing was replaced


# ------------------------------------------------------------------------------------------------------------------------
# 4. the restatement of rope_kv_store against the reference's own stores
# ------------------------------------------------------------------------------------------------------------------------
def _reference_stores(qkv, freqs, kc, vc, start_pos, H, Hkv):
    """fused_attn.py:253-267 on the CPU in float64: two with-pos rotations, then the permute / slice-assign stores
    (tests/test_gpu_attention_prefill.py::fill_ft_caches)."""
    xq, xk, xv = CP.split_qkv(qkv, H, Hkv)
    B, S, _, Dh = xk.shape
    q, _ = R.fused_rope_with_pos(xq, freqs)
    k, _ = R.fused_rope_with_pos(xk, freqs)
    kc, vc = kc.double().clone(), vc.clone()
    vc[:B, :, start_pos:start_pos + S, :] = xv.transpose(1, 2)
    kc[:B, :, :, start_pos:start_pos + S, :] = k.reshape(B, S, Hkv, Dh // 8, 8).permute(0, 2, 3, 1, 4)
    return q, kc, vc


@pytest.mark.parametrize("B,Bc,S,start,rot", [(1, 1, 5, 0, 64), (1, 2, 9, 7, 32), (2, 3, 6, 4, 64), (2, 2, 3, 13, 32)])
def test_restatement_reproduces_the_reference_stores(B, Bc, S, start, rot):
    H, Hkv, Dh, L = 4, 2, 64, 16
    g = torch.Generator().manual_seed(B * 100 + S)
    wide = torch.randn(B, S, (H + 2 * Hkv) * Dh + 16, generator=g)
    qkv = wide[:, :, 8:8 + (H + 2 * Hkv) * Dh]  # a strided slice of a wider buffer
    freqs = torch.randn(S, B, rot, generator=g)  # read flat: element (b, s, ., c) takes flat[(s * B + b) * rot + c]
    sent_k = torch.arange(Bc * Hkv * L * Dh, dtype=torch.float32).reshape(Bc, Hkv, Dh // 8, L, 8) + 0.5
    sent_v = -torch.arange(Bc * Hkv * L * Dh, dtype=torch.float32).reshape(Bc, Hkv, L, Dh) - 0.5
    q_ref, q_mag, k_ref, k_mag, v_new = CP.rope_kv_store(qkv, freqs, sent_k, sent_v, start, H, Hkv)
    q_want, k_want, v_want = _reference_stores(qkv, freqs, sent_k, sent_v, start, H, Hkv)
    assert torch.equal(q_ref, q_want) and torch.equal(k_ref, k_want) and torch.equal(v_new, v_want)
    # the flat-index quirk, directly: at B = 2 row (b, s) is rotated by the angles of flat row s * B + b, not by freqs[b, s]
    b, s, c = B - 1, S - 1, 3
    a = freqs.reshape(-1, rot)[s * B + b, c].double()
    x = qkv[b, s].view(H + 2 * Hkv, Dh)[H].double()  # KV head 0 of k
    assert abs(float(k_ref[b, 0, c // 8, start + s, c % 8] - (x[c] * a.cos() - x[c + rot // 2] * a.sin()))) < 1e-12
    # every other cache element is untouched: other positions, and the rows b >= B
    keep = torch.ones(L, dtype=torch.bool)
    keep[start:start + S] = False
    assert torch.equal(k_ref[:, :, :, keep], sent_k.double()[:, :, :, keep]) and torch.equal(v_new[:, :, keep], sent_v[:, :, keep])
    assert torch.equal(k_ref[B:], sent_k.double()[B:]) and torch.equal(v_new[B:], sent_v[B:])
    assert (k_mag[:, :, :, keep] == 0).all() and (k_mag[B:] == 0).all()
    assert not torch.equal(k_ref[:B, :, :, start:start + S], sent_k.double()[:B, :, :, start:start + S])
    # columns >= rot are copied
    if rot < Dh:
        xk = CP.split_qkv(qkv, H, Hkv)[1]
        got = k_ref[:B, :, rot // 8:, start:start + S].permute(0, 3, 1, 2, 4).reshape(B, S, Hkv, Dh - rot)
        assert torch.equal(got, xk[..., rot:].double())


def test_gather_and_scatter_of_the_ft_layout_are_inverse():
    B, Sk, Hkv, Dh = 2, 11, 3, 64
    k, v = torch.randn(B, Sk, Hkv, Dh), torch.randn(B, Sk, Hkv, Dh)
    kc, vc = CP.scatter_ft(k, v, B + 1, Sk + 9, 3)
    k2, v2 = CP.gather_ft(kc, vc, B, 3, Sk)
    assert torch.equal(k2, k) and torch.equal(v2, v)
    assert torch.isnan(kc).sum() == kc.numel() - k.numel() and torch.isnan(vc).sum() == vc.numel() - v.numel()
    k_off, v_off = CP.ft_offsets(B, Sk, Hkv, Dh, Sk + 9, 3)
    assert torch.equal(kc.view(-1)[k_off.reshape(-1)], k.reshape(-1)) and torch.equal(vc.view(-1)[v_off.reshape(-1)], v.reshape(-1))
