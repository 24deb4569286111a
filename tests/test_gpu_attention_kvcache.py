"""Attention over the natural-layout KV cache with per-sequence lengths read on the device (awq_attn_kvcache[_kv8],
csrc/awq_attn_splitkv_cdna4.hip): the ragged needle batches of tests/attn_kvcache_cases.py bit for bit through all three entry points
under a forced chunk of 64 keys, random ragged batches under the plan against the float64 oracle row by row and against the host-length
kernel pair bit for bit, inactive and too-short sequences, the FP8 cache, determinism and a poisoned workspace."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_kvcache_cases as K
from tests import attn_prefill_oracle as O
from tests import attn_splitkv_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _flash():
    llm_awq_amd.install_as_flash_attn()
    from flash_attn import flash_attn_with_kvcache  # the module name a decode engine imports

    return flash_attn_with_kvcache


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def chunk64():
    _capi.tune(attn_splitkv_chunk=K.CHUNK)
    yield
    _capi.tune(attn_splitkv_chunk=0)


def _assert_bits(out, want, what):
    assert torch.isfinite(out.float()).all(), what
    bad = out.cpu().view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:8].tolist())


# ------------------------------------------------------------------------------------------------------------------------
# needle batches: bit equality, every row, three entry points, chunk forced to 64 keys
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", K.CASES, ids=K.case_id)
def test_needle_batches_bit_exact_with_forced_chunks(spec, chunk64):
    batch = K.Batch(spec)
    s = batch.spec
    B, Sq, H, Dh = batch.q.shape
    assert ops.attn_kvcache_plan(B, H, s["Hkv"], Dh, Sq, batch.bound) == ((batch.bound + 63) // 64, 64)
    q, kc, vc, lens = (t.to(DEV) for t in (batch.q, batch.k_cache, batch.v_cache, batch.seqlens_k))
    out = ops.attn_kvcache(q, kc, vc, lens, batch.bound, batch.offset, batch.scale, batch.causal)
    torch.cuda.synchronize()
    assert out.shape == batch.target.shape and out.is_contiguous()
    _assert_bits(out, batch.target, "ops")
    for b, n in enumerate(batch.lens):
        if n is None:
            assert not out[b].view(torch.int16).any()  # exactly zero, not -0
    scale = Dh ** -0.5 if batch.scale is None else batch.scale
    _assert_bits(_engine().attn_kvcache(q, kc, vc, lens, batch.bound, batch.offset, scale, batch.causal), batch.target, "engine")
    # the shim takes total lengths and plans from the whole cache (bound + PAD rows): the targets do not depend on the bound
    total = lens + batch.offset
    _assert_bits(_flash()(q, kc, vc, cache_seqlens=total, softmax_scale=batch.scale, causal=batch.causal), batch.target, "flash_attn_with_kvcache")


def test_flash_attn_with_kvcache_takes_an_int_and_none(chunk64):
    spec = next(s for s in K.CASES if s["Sq"] == 8 and s["mode"] == "diag")
    batch = K.Batch(spec)
    q, kc, vc = (t.to(DEV) for t in (batch.q, batch.k_cache, batch.v_cache))
    f = _flash()
    b = batch.lens.index(72)
    out = f(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], cache_seqlens=72, causal=True)
    _assert_bits(out, batch.target[b:b + 1], "int cache_seqlens")
    whole = f(q[b:b + 1], kc[b:b + 1, :72], vc[b:b + 1, :72], causal=True)  # cache_seqlens=None: the whole cache, flash_attn_func
    _assert_bits(whole, batch.target[b:b + 1], "cache_seqlens=None")


# ------------------------------------------------------------------------------------------------------------------------
# random ragged batches under the plan: float64 row by row, and the host-length kernels bit for bit
# ------------------------------------------------------------------------------------------------------------------------
LENS, BOUND, PAD = (2111, 700, 300), 2304, 9
_REF = {}


def _ragged(Sq, dtype, Dh, lens=LENS, bound=BOUND, causal=True, H=8, Hkv=2):
    """The distributions of tests/test_gpu_attention_splitkv.py::make (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N) in a cache that holds NaN behind every
    sequence, and the float64 reference of every row; computed once per case, shared, never written to."""
    key = (Sq, dtype, Dh, lens, bound, causal)
    if key not in _REF:
        B = len(lens)
        g = torch.Generator(device=DEV).manual_seed(Sq * 31 + Dh + sum(lens))
        q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dtype)
        kc = torch.full((B, bound + PAD, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        vc = torch.full((B, bound + PAD, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        refs = []
        for b, n in enumerate(lens):
            kc[b, :n] = torch.randn(n, Hkv, Dh, generator=g, device=DEV).to(dtype)
            vc[b, :n] = (1 + 0.5 * torch.randn(n, Hkv, Dh, generator=g, device=DEV)).to(dtype)
            refs.append(O.attention(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], None, causal, stats=True) if n >= Sq or not causal else None)
        _REF[key] = (q, kc, vc, torch.tensor(lens, dtype=torch.int32, device=DEV), refs)
    return _REF[key]


def _check(out, ref, lim, what):
    assert torch.isfinite(out.float()).all(), what
    err = (out.double() - ref).abs()
    print(f"{what}: max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (what, int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_random_ragged_batch_within_the_bound_and_equal_to_the_host_length_kernels(Sq, dtype, Dh):
    """Every row within tests.attn_splitkv_oracle.bound of float64 with `splits` = the plan's (the combine visits at most that many
    partials; the empty ones add nothing).  The 2111-key row equals attn_splitkv on that sequence alone, bit for bit."""
    q, kc, vc, lens, refs = _ragged(Sq, dtype, Dh)
    B, _, H, _ = q.shape
    splits, chunk = ops.attn_kvcache_plan(B, H, 2, Dh, Sq, BOUND)
    assert (splits, chunk) == (3, 1024)  # no knob: the plan from the bound
    out = ops.attn_kvcache(q, kc, vc, lens - Sq, BOUND, Sq, None, True)  # lengths before the step, offset = Sq
    for b, n in enumerate(LENS):
        ref, Aw, qk = refs[b]
        _check(out[b:b + 1], ref, S.bound(ref, Aw, qk, dtype, n, Dh, Dh ** -0.5, splits), f"row {b} ({n} keys)")
    assert torch.equal(bits(_engine().attn_kvcache(q, kc, vc, lens, BOUND, 0, Dh ** -0.5, True)), bits(out))
    assert torch.equal(bits(_flash()(q, kc[:, :BOUND], vc[:, :BOUND], cache_seqlens=lens, causal=True)), bits(out))
    _capi.tune(attn_splitkv_chunk=chunk)
    try:
        assert ops.attn_splitkv_plan(1, H, 2, Dh, Sq, LENS[0], True) == (3, chunk)
        alone = ops.attn_splitkv(q[:1], kc[:1, :LENS[0]], vc[:1, :LENS[0]], None, True)
    finally:
        _capi.tune(attn_splitkv_chunk=0)
    assert torch.equal(bits(out[:1]), bits(alone))


def test_non_causal_ragged_batch_within_the_bound():
    lens, bound, Sq, Dh, dtype = (2500, 130), 2560, 4, 128, torch.bfloat16
    q, kc, vc, dl, refs = _ragged(Sq, dtype, Dh, lens=lens, bound=bound, causal=False)
    splits = ops.attn_kvcache_plan(2, 8, 2, Dh, Sq, bound)[0]
    assert splits == 3
    out = ops.attn_kvcache(q, kc, vc, dl, bound, 0, None, False)
    for b, n in enumerate(lens):
        ref, Aw, qk = refs[b]
        _check(out[b:b + 1], ref, S.bound(ref, Aw, qk, dtype, n, Dh, Dh ** -0.5, splits), f"non-causal row {b}")
    assert torch.equal(bits(_flash()(q, kc[:, :bound], vc[:, :bound], cache_seqlens=dl, causal=False)), bits(out))


def test_inactive_and_too_short_sequences_return_zeros_and_never_nan(chunk64):
    """Lengths 2 < Sq (rows 0 and 1 have a negative causal limit), 0, bound + 1 and a corrupt negative one beside a live sequence."""
    Sq, Dh, bound, dtype = 4, 64, 128, torch.float16
    q, kc, vc, _, refs = _ragged(Sq, dtype, Dh, lens=(2, 70, 70, 70, 70), bound=bound)
    lens = torch.tensor([2, 0, bound + 1, -(2 ** 31), 70], dtype=torch.int32, device=DEV)
    out = ops.attn_kvcache(q, kc, vc, lens, bound, 0, None, True)
    assert torch.isfinite(out.float()).all()
    assert not out[1:4].view(torch.int16).any() and not out[0, :2].view(torch.int16).any()
    ref, Aw, qk = refs[4]
    _check(out[4:5], ref, S.bound(ref, Aw, qk, dtype, 70, Dh, Dh ** -0.5, 2), "the live row")
    # rows 2 and 3 of the two-key sequence are a square causal call of their own
    ref2, Aw2, qk2 = O.attention(q[:1, 2:], kc[:1, :2], vc[:1, :2], None, True, stats=True)
    _check(out[:1, 2:], ref2, S.bound(ref2, Aw2, qk2, dtype, 2, Dh, Dh ** -0.5, 2), "rows behind the negative limits")
    # the largest offset: no overflow into an active length
    assert not ops.attn_kvcache(q, kc, vc, torch.full((5,), 2 ** 31 - 1, dtype=torch.int32, device=DEV), bound, Sq, None, True).view(torch.int16).any()


# ------------------------------------------------------------------------------------------------------------------------
# FP8 cache: bit-equal to the T form on the dequantised caches
# ------------------------------------------------------------------------------------------------------------------------
def _fp8_pair(q, kc, vc, lens, bound, offset, scale, causal):
    kq, ks = ops.kv8_quant(kc)
    vq, vs = ops.kv8_quant(vc)
    got = ops.attn_kvcache(q, kq, vq, lens, bound, offset, scale, causal, k_scale=ks, v_scale=vs)
    want = ops.attn_kvcache(q, ops.kv8_dequant(kq, ks, q.dtype), ops.kv8_dequant(vq, vs, q.dtype), lens, bound, offset, scale, causal)
    return got, want, (kq, vq, ks, vs)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda x: str(x).replace("torch.", ""))
def test_fp8_needle_batch_equals_the_t_form_on_the_dequantised_cache(dtype, chunk64):
    spec = next(s for s in K.CASES if s["Sq"] == 8 and s["mode"] == "scatter" and s["dtype"] == dtype)
    batch = K.Batch(spec)
    q, kc, vc, lens = (t.to(DEV) for t in (batch.q, batch.k_cache, batch.v_cache, batch.seqlens_k))
    got, want, (kq, vq, ks, vs) = _fp8_pair(q, kc, vc, lens, batch.bound, batch.offset, batch.scale, True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(bits(got), bits(want))
    Dh = q.shape[3]
    eng = _engine().attn_kvcache_kv8(q, kq, vq, ks, vs, lens, batch.bound, batch.offset, Dh ** -0.5, True)
    assert torch.equal(bits(eng), bits(got))


def test_fp8_random_ragged_batch_equals_the_t_form_on_the_dequantised_cache():
    q, kc, vc, lens, _ = _ragged(4, torch.bfloat16, 128)
    got, want, _ = _fp8_pair(q, kc, vc, lens, BOUND, 0, None, True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------------------------------
# determinism, a poisoned workspace
# ------------------------------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bits_and_a_nan_workspace_changes_nothing():
    Sq, dtype, Dh = 4, torch.float16, 64
    q, kc, vc, lens, _ = _ragged(Sq, dtype, Dh)
    a = ops.attn_kvcache(q, kc, vc, lens, BOUND, 0, None, True)
    b = ops.attn_kvcache(q, kc, vc, lens, BOUND, 0, None, True)
    assert torch.equal(bits(a), bits(b))
    B, _, H, _ = q.shape
    L = _capi.lib()
    wsb = L.awq_attn_kvcache_workspace_bytes(B, H, 2, Dh, Sq, BOUND)
    assert wsb == B * H * Sq * 3 * (Dh + 2) * 4
    ws = torch.full((wsb // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full_like(a, float("nan"))
    with torch.cuda.device(q.device):
        _capi.check(L.awq_attn_kvcache(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), B, Sq, lens.data_ptr(), 0, BOUND, kc.shape[1], H, 2,
                                       Dh, q.stride(0), q.stride(1), kc.stride(0), kc.stride(1), vc.stride(0), vc.stride(1), Dh ** -0.5, 1, 0,
                                       ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(a))
    # the short sequences left their later splits empty: m = -inf, l = 0, and an O that nobody wrote or read
    n = B * H * Sq * 3
    m = ws[n * Dh:n * Dh + n].view(B, 2, Sq * (H // 2), 3)
    assert torch.isinf(m[1:, :, :, 1:]).all() and (m[1:, :, :, 1:] < 0).all() and torch.isfinite(m[0]).all() and torch.isfinite(m[:, :, :, 0]).all()
    assert not ws[n * Dh + n:].view(B, 2, -1, 3)[1:, :, :, 1:].any()
