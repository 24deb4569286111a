"""The FP8 KV cache on the MI355X (csrc/awq_kv8.hpp, awq_attn_kv8_cdna4.hip and the Kv8 instantiations of the two attention kernels).
No tolerance anywhere: the store launch against the numpy restatement of the format (tests/kv8_oracle.py) applied to what
rope_kv_store_natural stores, byte for byte; both attention kernels against the T-cache kernels on the dequantised tensors, bit for bit;
the module against a restatement assembled from those pieces.  The quality figure at the end is printed, not asserted."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import kv8_oracle as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_T = {"f16": torch.float16, "bf16": torch.bfloat16}


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


def T(x, dtype):
    """float32 numpy holding T values -> GPU tensor of T"""
    return torch.from_numpy(K.to_bits(x, dtype).view(np.int16)).view(TORCH_T[dtype]).to(DEV)


def np_of(t, dtype):
    """GPU tensor of T -> float32 numpy"""
    return K.from_bits(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dtype)


@pytest.fixture
def chunk64():
    _capi.tune(attn_splitkv_chunk=K.CHUNK)
    yield
    _capi.tune(attn_splitkv_chunk=0)


@pytest.fixture
def q_tile():
    yield lambda rows: _capi.tune(attn_prefill_rows=rows)
    _capi.tune(attn_prefill_rows=0)


# ------------------------------------------------------------------------------------------------------------------------
# the store launch
# ------------------------------------------------------------------------------------------------------------------------
CODE_SENTINEL, SCALE_SENTINEL = 0xA5, -7.25


@pytest.mark.parametrize("case", K.STORE_CASES, ids=K.store_id)
def test_store_writes_the_oracles_codes_and_scales_and_nothing_else(case):
    E = _engine()
    B, Bc, H, Hkv, L = (K.STORE[n] for n in ("B", "Bc", "H", "Hkv", "lmax"))
    S, Dh, dt, start = case["S"], case["Dh"], case["dtype"], case["start"]
    dtype = TORCH_T[dt]
    qkv_np, freqs_np, plain, k_in, v_in = K.store_inputs(case)
    W = qkv_np.shape[-1]
    wide = torch.full((B, S + 1, W + 24), float("nan"), dtype=dtype, device=DEV)  # a strided view, NaN rows and columns around it
    qkv = wide[:, :S, 8:8 + W]
    qkv.copy_(T(qkv_np, dt))
    freqs = torch.from_numpy(freqs_np).to(DEV)
    # what rope_kv_store_natural stores, and its q
    kt = torch.zeros(Bc, L, Hkv, Dh, dtype=dtype, device=DEV)
    vt = torch.zeros(Bc, L, Hkv, Dh, dtype=dtype, device=DEV)
    q_want = ops.rope_kv_store_natural(qkv, freqs, kt, vt, start, H, Hkv)
    k_st, v_st = np_of(kt[:B, start:start + S], dt), np_of(vt[:B, start:start + S], dt)
    assert np.array_equal(k_st[plain], k_in[plain]) and np.array_equal(v_st, v_in)  # the K needles reach the quantiser as they were built
    assert not np.array_equal(k_st[~plain], k_in[~plain]) or plain.all()
    want_kc = np.full((Bc, L, Hkv, Dh), CODE_SENTINEL, np.uint8)
    want_vc = want_kc.copy()
    want_ks = np.full((Bc, L, Hkv), SCALE_SENTINEL, np.float32)
    want_vs = want_ks.copy()
    want_kc[:B, start:start + S], want_ks[:B, start:start + S] = K.quant(k_st)
    want_vc[:B, start:start + S], want_vs[:B, start:start + S] = K.quant(v_st)
    for fn, cache_dtype in ((ops.rope_kv_store_natural_fp8, torch.float8_e4m3fn), (E.rope_kv_store_natural_fp8, torch.uint8)):
        kc = torch.full((Bc, L, Hkv, Dh), CODE_SENTINEL, dtype=torch.uint8, device=DEV).view(cache_dtype)
        vc = torch.full((Bc, L, Hkv, Dh), CODE_SENTINEL, dtype=torch.uint8, device=DEV).view(cache_dtype)
        ks = torch.full((Bc, L, Hkv), SCALE_SENTINEL, device=DEV)
        vs = torch.full((Bc, L, Hkv), SCALE_SENTINEL, device=DEV)
        q_out = fn(qkv, freqs, kc, vc, ks, vs, start, H, Hkv)
        torch.cuda.synchronize()
        assert q_out.shape == (B, S, H, Dh) and q_out.is_contiguous()
        assert torch.equal(bits(q_out), bits(q_want))
        for name, got, want in (("k codes", kc.view(torch.uint8), want_kc), ("v codes", vc.view(torch.uint8), want_vc),
                                ("k scales", ks.view(torch.int32), want_ks.view(np.int32)), ("v scales", vs.view(torch.int32), want_vs.view(np.int32))):
            got = got.cpu().numpy()
            bad = np.argwhere(got != want)
            assert not len(bad), (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])  # window and sentinels at once


@pytest.mark.parametrize("dt", K.DTYPES)
def test_store_with_a_partial_rotation(dt):
    """rot_dim = Dh / 2: the lanes of the copied chunks and those of the rotated chunks of one head row meet at the row's amax."""
    B, Bc, H, Hkv, L, S, Dh, start = 2, 2, 4, 2, 16, 5, 128, 3
    dtype = TORCH_T[dt]
    g = torch.Generator(device=DEV).manual_seed(17)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * Dh, generator=g, device=DEV)
    qkv[..., H * Dh + Dh - 1::Dh] *= 30  # the amax of every K / V row sits in a copied column
    qkv = qkv.to(dtype)
    freqs = (50.0 * torch.randn(S, B, Dh // 2, generator=g, device=DEV)).contiguous()
    kt, vt = torch.zeros(Bc, L, Hkv, Dh, dtype=dtype, device=DEV), torch.zeros(Bc, L, Hkv, Dh, dtype=dtype, device=DEV)
    q_want = ops.rope_kv_store_natural(qkv, freqs, kt, vt, start, H, Hkv)
    kc = torch.zeros(Bc, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    vc = torch.zeros(Bc, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    ks, vs = torch.zeros(Bc, L, Hkv, device=DEV), torch.zeros(Bc, L, Hkv, device=DEV)
    q_out = ops.rope_kv_store_natural_fp8(qkv, freqs, kc, vc, ks, vs, start, H, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(bits(q_out), bits(q_want))
    for cache, scale, t in ((kc, ks, kt), (vc, vs, vt)):
        codes, s = K.quant(np_of(t[:, start:start + S], dt))
        assert np.array_equal(cache[:, start:start + S].view(torch.uint8).cpu().numpy(), codes)
        assert np.array_equal(scale[:, start:start + S].cpu().numpy().view(np.uint32), s.view(np.uint32))
        assert not cache[:, :start].view(torch.uint8).any() and not cache[:, start + S:].view(torch.uint8).any()


def test_store_refuses_what_does_not_fit():
    E = _engine()
    B, S, H, Hkv, Dh, L = 2, 8, 4, 2, 64, 16
    qkv = torch.zeros(B, S, (H + 2 * Hkv) * Dh, dtype=torch.float16, device=DEV)
    fr = torch.zeros(S, B, Dh, device=DEV)
    kc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    vc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    ks, vs = torch.zeros(B, L, Hkv, device=DEV), torch.zeros(B, L, Hkv, device=DEV)
    with pytest.raises(RuntimeError, match="do not fit"):
        E.rope_kv_store_natural_fp8(qkv, fr, kc, vc, ks, vs, 9, H, Hkv)
    with pytest.raises(_capi.AwqNativeError):
        ops.rope_kv_store_natural_fp8(qkv, fr, kc, vc, ks, vs, 9, H, Hkv)
    with pytest.raises(RuntimeError, match="k_cache must be float8_e4m3fn or uint8"):
        E.rope_kv_store_natural_fp8(qkv, fr, kc.view(torch.uint8).half(), vc, ks, vs, 0, H, Hkv)
    with pytest.raises(RuntimeError, match="v_scale must be float32"):
        E.rope_kv_store_natural_fp8(qkv, fr, kc, vc, ks, vs.half(), 0, H, Hkv)
    with pytest.raises(RuntimeError, match="k_scale must be"):
        E.rope_kv_store_natural_fp8(qkv, fr, kc, vc, ks[:, :8].contiguous(), vs, 0, H, Hkv)
    with pytest.raises(ValueError, match="k_cache must be float8_e4m3fn or uint8"):
        ops.rope_kv_store_natural_fp8(qkv, fr, kc.view(torch.uint8).half(), vc, ks, vs, 0, H, Hkv)
    torch.cuda.synchronize()
    assert not kc.view(torch.uint8).any() and not ks.any() and not vs.any()


# ------------------------------------------------------------------------------------------------------------------------
# the attention kernels: the T-cache kernels on the dequantised tensors, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def _cache(Sq, Sk, G, Dh, dt, as_fp8):
    """q and the [:B, :Sk] slices of the longer FP8 cache of the oracle's case (NaN codes and NaN scales behind row Sk), on the GPU,
    and the dequantised T tensors the reference kernels read."""
    d = K.attn_inputs(Sq, Sk, G, Dh, dt)
    dtype = TORCH_T[dt]
    q = T(d["q"], dt)
    code = lambda a: (torch.from_numpy(a).to(DEV).view(torch.float8_e4m3fn) if as_fp8 else torch.from_numpy(a).to(DEV))[:, :Sk]
    k8, v8 = code(d["kc"]), code(d["vc"])
    ks, vs = torch.from_numpy(d["ks"]).to(DEV)[:, :Sk], torch.from_numpy(d["vs"]).to(DEV)[:, :Sk]
    assert not k8.is_contiguous() and not ks.is_contiguous()
    kd, vd = ops.kv8_dequant(k8, ks, dtype), ops.kv8_dequant(v8, vs, dtype)
    return q, k8, v8, ks, vs, kd, vd


def _same(got, want):
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.is_contiguous()
    assert torch.isfinite(got.float()).all()
    bad = bits(got) != bits(want)
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dt", K.DTYPES)
def test_torch_quant_on_the_gpu_is_the_oracles(dt, Dh):
    """ops.kv8_quant states the format on any device: on the GPU too its division and its cast give the oracle's codes and scales."""
    needles, _ = K.needle_block(dt, 2, Dh)
    x = np.concatenate([needles, K.random_block(dt, 40, 2, Dh, seed=Dh)])
    codes, scale = K.quant(x)
    tc, ts = ops.kv8_quant(T(x, dt))
    assert tc.is_cuda and tc.dtype == torch.float8_e4m3fn
    assert np.array_equal(tc.view(torch.uint8).cpu().numpy(), codes)
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), scale.view(np.uint32))


def test_torch_dequant_on_the_gpu_is_the_oracles():
    for dt in K.DTYPES:
        d = K.attn_inputs(8, 193, 4, 64, dt)
        q, k8, v8, ks, vs, kd, vd = _cache(8, 193, 4, 64, dt, True)
        assert np.array_equal(np_of(kd, dt).view(np.uint32), K.dequant(d["kc"][:, :193], d["ks"][:, :193], dt).view(np.uint32))
        assert np.array_equal(np_of(vd, dt).view(np.uint32), K.dequant(d["vc"][:, :193], d["vs"][:, :193], dt).view(np.uint32))


@pytest.mark.parametrize("case", K.SPLIT_FORCED, ids=K.attn_id)
def test_splitkv_kv8_is_splitkv_on_the_dequantised_cache_with_forced_chunks(case, chunk64):
    Sq, Sk, G, causal, Dh, dt = (case[n] for n in ("Sq", "Sk", "G", "causal", "Dh", "dtype"))
    splits, chunk = ops.attn_splitkv_plan(K.ATTN_B, G * K.ATTN_HKV, K.ATTN_HKV, Dh, Sq, Sk, causal)
    assert chunk == 64 and splits == (Sk + 63) // 64 > 1  # the split kernels run
    q, k8, v8, ks, vs, kd, vd = _cache(Sq, Sk, G, Dh, dt, as_fp8=(G == 1))
    want = ops.attn_splitkv(q, kd, vd, None, causal)
    _same(ops.attn_splitkv_kv8(q, k8, v8, ks, vs, None, causal), want)
    _same(_engine().attn_splitkv_kv8(q, k8, v8, ks, vs, Dh ** -0.5, causal), want)


@pytest.mark.parametrize("case", K.SPLIT_PLAN, ids=K.attn_id)
def test_splitkv_kv8_under_the_plan(case):
    Sq, Sk, G, causal, Dh, dt = (case[n] for n in ("Sq", "Sk", "G", "causal", "Dh", "dtype"))
    assert ops.attn_splitkv_plan(K.ATTN_B, G * K.ATTN_HKV, K.ATTN_HKV, Dh, Sq, Sk, causal)[0] > 1
    q, k8, v8, ks, vs, kd, vd = _cache(Sq, Sk, G, Dh, dt, as_fp8=(Sq == 1))
    want = ops.attn_splitkv(q, kd, vd, None, causal)
    _same(ops.attn_splitkv_kv8(q, k8, v8, ks, vs, None, causal), want)
    _same(ops.attn_kv8(q, k8, v8, ks, vs, None, causal), want)


@pytest.mark.parametrize("case", K.ONEPASS, ids=K.attn_id)
def test_prefill_kv8_is_prefill_on_the_dequantised_cache_at_every_q_tile(case, q_tile):
    rows, Dh, dt = case["rows"], case["Dh"], case["dtype"]
    E = _engine()
    q_tile(rows)
    for Sq, Sk, causal in K.ONEPASS_SHAPES:
        for G in (1, 4):
            assert ops.attn_prefill_plan(K.ATTN_B, G * K.ATTN_HKV, K.ATTN_HKV, Dh, Sq, Sk, causal)[0] == rows
            q, k8, v8, ks, vs, kd, vd = _cache(Sq, Sk, G, Dh, dt, as_fp8=causal)
            want = E.attn_prefill(q, kd, vd, Dh ** -0.5, causal)
            _same(ops.attn_prefill_kv8(q, k8, v8, ks, vs, None, causal), want)
            if G == 4:
                _same(E.attn_prefill_kv8(q, k8, v8, ks, vs, Dh ** -0.5, causal), want)
                _same(ops.attn_kv8(q, k8, v8, ks, vs, None, causal), want)  # no knob, Sk < 2048: the plan does not split


def test_attn_kv8_takes_the_split_entry_exactly_where_the_plan_splits(monkeypatch):
    calls = []
    real = ops._attn_kv8  # the one place both entries are called from: its first argument names the C entry
    monkeypatch.setattr(ops, "_attn_kv8", lambda entry, *a, **kw: (calls.append("attn_" + entry + "_kv8"), real(entry, *a, **kw))[1])
    try:
        for knob, (Sq, Sk, G), expect in ((0, (8, 193, 4), "attn_prefill_kv8"), (64, (8, 193, 4), "attn_splitkv_kv8"),
                                          (0, (1, 2049, 4), "attn_splitkv_kv8"), (64, (33, 193, 4), "attn_prefill_kv8")):  # 33 * 4 rows > 128
            _capi.tune(attn_splitkv_chunk=knob)
            q, k8, v8, ks, vs, kd, vd = _cache(Sq, Sk, G, 128, "bf16", True)
            split = ops.attn_splitkv_plan(K.ATTN_B, G * K.ATTN_HKV, K.ATTN_HKV, 128, Sq, Sk, True)[0] > 1
            assert split == (expect == "attn_splitkv_kv8")
            del calls[:]
            out = ops.attn_kv8(q, k8, v8, ks, vs, None, True)
            assert calls == [expect], (knob, Sq, Sk, calls)
            _same(out, ops.flash_attn_func(q, kd, vd, None, True))  # which routes by the same plan
    finally:
        _capi.tune(attn_splitkv_chunk=0)


def test_kv8_attention_refuses_wrong_tensors():
    E = _engine()
    q, k8, v8, ks, vs, kd, vd = _cache(8, 193, 4, 64, "f16", True)
    with pytest.raises(RuntimeError, match="k must be float8_e4m3fn or uint8"):
        E.attn_splitkv_kv8(q, kd, v8, ks, vs, 0.125, True)
    with pytest.raises(RuntimeError, match="v_scale must be float32"):
        E.attn_prefill_kv8(q, k8, v8, ks, vs.half(), 0.125, True)
    with pytest.raises(RuntimeError, match="k_scale must be"):
        E.attn_prefill_kv8(q, k8, v8, ks[:, :100], vs, 0.125, True)
    with pytest.raises(RuntimeError, match="head dim"):
        E.attn_prefill_kv8(q[..., :32].contiguous(), k8[..., :32].contiguous(), v8[..., :32].contiguous(), ks, vs, 0.125, True)
    with pytest.raises(ValueError, match="v must be float8_e4m3fn or uint8"):
        ops.attn_kv8(q, k8, vd, ks, vs, None, True)
    with pytest.raises(ValueError, match="k_scale"):
        ops.attn_kv8(q, k8, v8, ks.double(), vs, None, True)


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
FLOW = dict(B=1, H=4, Hkv=2, Dh=128, L=96, steps=(70, 5, 1, 1, 1), forced=3)  # the step of index 3 runs under the forced chunk


def _freqs(start, n, Dh, base=10000.0):
    inv = 1.0 / (base ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(start, start + n, device=DEV).float(), inv)
    return torch.cat([f, f], -1)[None].contiguous()


def _inputs(dtype, steps, seed=3):
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
    return QuantLlamaAttentionFused(H * Dh, H, FLOW["L"], torch.nn.Identity(), torch.nn.Identity(), DEV, args, **kw)


@pytest.mark.parametrize("dt", K.DTYPES)
def test_module_with_the_fp8_cache_is_its_restatement_bit_for_bit(dt):
    """The restatement, from existing pieces: rope_kv_store_natural into T caches, the oracle's quant -> dequant of the cached history,
    flash_attn_func on the result.  A kv_dtype=None module beside it still gives the bits of its own restatement (no quantisation)."""
    dtype = TORCH_T[dt]
    B, H, Hkv, Dh, L = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"], FLOW["L"]
    xs = _inputs(dtype, FLOW["steps"])
    m8, mt = _module(kv_layout="natural", kv_dtype="fp8"), _module(kv_layout="natural")
    assert m8.cache_k.dtype == torch.float8_e4m3fn and tuple(m8.cache_k_scale.shape) == (1, L, Hkv) and not hasattr(mt, "cache_k_scale")
    ck, cv = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV), torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
    pos = 0
    try:
        for i, x in enumerate(xs):
            S = x.shape[1]
            fr = _freqs(pos, S, Dh)
            _capi.tune(attn_splitkv_chunk=64 if i == FLOW["forced"] else 0)
            assert (ops.attn_splitkv_plan(B, H, Hkv, Dh, S, pos + S, True)[0] > 1) == (i == FLOW["forced"])
            got8 = m8(x, pos, fr, None, chunk_prefilling=(S > 1 and pos > 0))
            gott = mt(x, pos, fr, None, chunk_prefilling=(S > 1 and pos > 0))
            xq = ops.rope_kv_store_natural(x, fr, ck, cv, pos, H, Hkv)
            end = pos + S
            wantt = ops.flash_attn_func(xq, ck[:B, :end], cv[:B, :end], None, True).view(B, S, -1)
            kc, ks, vc, vs, kd, vd = K.cache_roundtrip(np_of(ck[:B, :end], dt), np_of(cv[:B, :end], dt), dt)
            want8 = ops.flash_attn_func(xq, T(kd, dt), T(vd, dt), None, True).view(B, S, -1)
            torch.cuda.synchronize()
            assert got8.shape == (B, S, H * Dh)
            assert torch.equal(bits(gott), bits(wantt)), (i, pos, S)
            assert torch.equal(bits(got8), bits(want8)), (i, pos, S, int((bits(got8) != bits(want8)).sum()))
            assert not torch.equal(bits(got8), bits(gott))  # the quantisation is visible
            pos = end
    finally:
        _capi.tune(attn_splitkv_chunk=0)
    assert pos == 78 and m8.cache_k.dtype == torch.float8_e4m3fn and m8.cache_k_scale.dtype == torch.float32 and mt.cache_k.dtype == dtype
    assert np.array_equal(m8.cache_k[:B, :pos].view(torch.uint8).cpu().numpy(), kc) and np.array_equal(m8.cache_v[:B, :pos].view(torch.uint8).cpu().numpy(), vc)
    assert np.array_equal(m8.cache_k_scale[:B, :pos].cpu().numpy().view(np.uint32), ks.view(np.uint32))
    assert np.array_equal(m8.cache_v_scale[:B, :pos].cpu().numpy().view(np.uint32), vs.view(np.uint32))
    assert not m8.cache_k[:, pos:].view(torch.uint8).any() and not m8.cache_k_scale[:, pos:].any()
    assert torch.equal(bits(mt.cache_k), bits(ck)) and torch.equal(bits(mt.cache_v), bits(cv))


# ------------------------------------------------------------------------------------------------------------------------
# graph capture: store + attention in one graph, one stream
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Dh", [("f16", 64), ("bf16", 128)])
def test_store_and_attention_replay_from_one_graph(dt, Dh, chunk64):
    dtype = TORCH_T[dt]
    B, H, Hkv, L, pos = 1, 8, 2, 256, 192  # one token over 193 keys, chunk 64: the split kernels and their workspace
    hist = K.attn_inputs(1, pos, 4, Dh, dt)
    kc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    vc = torch.zeros(B, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    ks, vs = torch.zeros(B, L, Hkv, device=DEV), torch.zeros(B, L, Hkv, device=DEV)
    kc[:, :pos] = torch.from_numpy(hist["kc"][:B, :pos]).to(DEV).view(torch.float8_e4m3fn)
    vc[:, :pos] = torch.from_numpy(hist["vc"][:B, :pos]).to(DEV).view(torch.float8_e4m3fn)
    ks[:, :pos], vs[:, :pos] = torch.from_numpy(hist["ks"][:B, :pos]).to(DEV), torch.from_numpy(hist["vs"][:B, :pos]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(21)
    x = torch.randn(B, 1, (H + 2 * Hkv) * Dh, generator=g, device=DEV).to(dtype)
    fr = _freqs(pos, 1, Dh)
    assert ops.attn_splitkv_plan(B, H, Hkv, Dh, 1, pos + 1, True)[0] == 4

    def step():
        q = ops.rope_kv_store_natural_fp8(x, fr, kc, vc, ks, vs, pos, H, Hkv)
        return ops.attn_kv8(q, kc[:, :pos + 1], vc[:, :pos + 1], ks[:, :pos + 1], vs[:, :pos + 1], None, True)
    eager = step().clone()
    row = (kc[:, pos].view(torch.uint8).clone(), ks[:, pos].clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        o = step()
    for _ in range(2):
        o.fill_(float("nan"))
        kc[:, pos].view(torch.uint8).fill_(0x7F)  # the replay stores the new token again
        ks[:, pos].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(o), bits(eager))
        assert torch.equal(kc[:, pos].view(torch.uint8), row[0]) and torch.equal(ks[:, pos], row[1])


# ------------------------------------------------------------------------------------------------------------------------
# the quality figure: reported, not asserted (DESIGN.md carries the numbers)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", K.DTYPES)
def test_report_the_difference_to_the_t_cache(dt):
    from tests.test_gpu_attention_splitkv import make

    dtype = TORCH_T[dt]
    for Sk in (2049, 8193):
        B, Hkv, G, Dh = (2, 2, 4, 128) if Sk < 8000 else (1, 1, 8, 128)
        q, k, v = make(B, G * Hkv, Hkv, Dh, 1, Sk, dtype, seed=31 + Sk + Dh)
        (k8, ks), (v8, vs) = ops.kv8_quant(k), ops.kv8_quant(v)
        ref = ops.flash_attn_func(q, k, v, None, True).float()
        out = ops.attn_kv8(q, k8, v8, ks, vs, None, True).float()
        torch.cuda.synchronize()
        diff = (out - ref).abs()
        print(f"kv8 quality {dt} Sk={Sk}: max |d| = {float(diff.max()):.3e}, rms d = {float(diff.pow(2).mean().sqrt()):.3e}, "
              f"rms out = {float(ref.pow(2).mean().sqrt()):.3e}")
        assert torch.isfinite(out).all()
