"""Prompt chunks of any length on the device-length and paged KV caches (awq_attn_prefill_kvcache[_kv8], awq_attn_prefill_paged[_kv8];
csrc/awq_attn_prefill_cdna4.hip): the needle batches of tests/attn_prefill_kvcache_cases.py bit for bit, bit-identity to the host-length
one-pass kernel per sequence at every q tile, random ragged batches against float64, table entries that must never be read, determinism,
one captured graph of store + attention across a page edge, and the module: a prompt in one call against the same prompt in pieces,
against the host-position forward, on the FP8 cache and as a ragged batch."""
import os
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
from llm_awq_amd.paged_kv import PageTable
from tests import attn_prefill_kvcache_cases as C
from tests import attn_prefill_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


def _assert_bits(out, want, what):
    assert torch.isfinite(out.float()).all(), what
    bad = out.cpu().view(torch.int16) != want.cpu().view(torch.int16)
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.fixture
def q_tile():
    """Forces the q tile of the one-pass kernel (knob attn_prefill_rows) and restores the plan's choice afterwards."""
    had = os.environ.get("AWQ_TUNING")
    yield lambda rows: _capi.tune(attn_prefill_rows=rows)
    _capi.tune(attn_prefill_rows=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def _quant(kp, vp):
    """FP8 pools of T pools (a NaN row has no scale; nothing that holds no key is read anyway)."""
    kq, ks = ops.kv8_quant(kp.nan_to_num(0.0))
    vq, vs = ops.kv8_quant(vp.nan_to_num(0.0))
    return kq, vq, ks, vs


# ------------------------------------------------------------------------------------------------------------------------
# needle batches: bit equality with the CPU targets, dense and paged, T and FP8
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_needle_batches_bit_exact_on_the_dense_caches(spec):
    pb = C.PrefillBatch(spec)
    q, kc, vc, lens = (t.to(DEV) for t in (pb.q, pb.k_cache, pb.v_cache, pb.seqlens_k))
    out = ops.attn_prefill_kvcache(q, kc, vc, lens, pb.bound, pb.offset, pb.scale, pb.causal)
    torch.cuda.synchronize()
    assert out.shape == pb.target.shape and out.is_contiguous()
    _assert_bits(out, pb.target, "ops")
    for b, n in enumerate(pb.lens):
        if not pb.active(n):
            assert not out[b].view(torch.int16).any()  # exactly zero, not -0
    scale = q.shape[3] ** -0.5 if pb.scale is None else pb.scale
    _assert_bits(_engine().attn_prefill_kvcache(q, kc, vc, lens, pb.bound, pb.offset, scale, pb.causal), pb.target, "engine")
    # FP8: the T form on the dequantised caches, bit for bit -- and the CPU restatement on them (K survives the quantisation exactly, so the
    # weights stay one-hot; a pair's mean of two dequantised rows may be a rounding tie, which float64's residual weights decide otherwise)
    kq, vq, ks, vs = _quant(kc, vc)
    got = ops.attn_prefill_kvcache(q, kq, vq, lens, pb.bound, pb.offset, pb.scale, pb.causal, k_scale=ks, v_scale=vs)
    kd, vd = ops.kv8_dequant(kq, ks, pb.dtype), ops.kv8_dequant(vq, vs, pb.dtype)
    _assert_bits(got, ops.attn_prefill_kvcache(q, kd, vd, lens, pb.bound, pb.offset, pb.scale, pb.causal), "fp8 against T on the dequantised caches")
    _assert_bits(_engine().attn_prefill_kvcache_kv8(q, kq, vq, ks, vs, lens, pb.bound, pb.offset, scale, pb.causal), got, "engine fp8")
    if pb.mode != "pair":
        assert torch.equal(bits(kd.cpu()[~torch.isnan(pb.k_cache)]), bits(pb.k_cache[~torch.isnan(pb.k_cache)]))
        pb.k_cache, pb.v_cache = kd.cpu(), vd.cpu()
        _assert_bits(got, C.dense(pb), "fp8 against the CPU restatement")


@pytest.mark.parametrize("spec", C.PAGED_CASES, ids=C.case_id)
def test_needle_batches_bit_exact_through_the_table(spec):
    pp = C.PagedPrefill(spec)
    pb = pp.batch
    q, lens, kp, vp = (t.to(DEV) for t in (pb.q, pb.seqlens_k, pp.k_pool, pp.v_pool))
    table = pp.table_full.to(DEV)[:, :pp.pps]  # the row stride stays wider than pages_per_seq
    assert table.stride(0) == pp.pps + C.PAD_COLS
    out = ops.attn_prefill_paged(q, kp, vp, table, lens, pb.bound, pb.offset, pb.scale, pb.causal)
    torch.cuda.synchronize()
    _assert_bits(out, pb.target, "ops")
    scale = q.shape[3] ** -0.5 if pb.scale is None else pb.scale
    _assert_bits(_engine().attn_prefill_paged(q, kp, vp, table, lens, pb.bound, pb.offset, scale, pb.causal), pb.target, "engine")
    kd, vd = (t.to(DEV) for t in pp.dense())
    _assert_bits(ops.attn_prefill_kvcache(q, kd, vd, lens, pb.bound, pb.offset, pb.scale, pb.causal), out, "dense gather")
    kq, vq, ks, vs = _quant(kp, vp)
    got = ops.attn_prefill_paged(q, kq, vq, table, lens, pb.bound, pb.offset, pb.scale, pb.causal, k_scale=ks, v_scale=vs)
    deq = ops.kv8_dequant(kq, ks, pb.dtype), ops.kv8_dequant(vq, vs, pb.dtype)
    _assert_bits(got, ops.attn_prefill_paged(q, *deq, table, lens, pb.bound, pb.offset, pb.scale, pb.causal), "fp8 against T on the dequantised pools")
    _assert_bits(_engine().attn_prefill_paged_kv8(q, kq, vq, ks, vs, table, lens, pb.bound, pb.offset, scale, pb.causal), got, "engine fp8")
    if pb.mode != "pair":
        _assert_bits(got, C.paged(pp, pools=tuple(t.cpu() for t in deq)), "fp8 against the CPU restatement")


# ------------------------------------------------------------------------------------------------------------------------
# random ragged batches (shared by the tests below, never written to): Sq 200, histories up to 700, bound 1024
# ------------------------------------------------------------------------------------------------------------------------
OVER = 900   # a history that takes its sequence beyond the bound: inactive (an entry of -1 would be a sequence of SQ - 1 keys here)
SQ, HIST, BOUND, PS, PAD = 200, (700, 333, 0, 57, OVER), 1024, 128, 9
COMBOS = [(torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)]
_REF = {}


def _ragged(dtype, Dh, H=8, Hkv=2):
    """q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N in a cache that holds NaN behind every sequence, the same keys in a shuffled pool of 128-key pages
    whose unused rows are NaN (table entries behind a live range: the NaN poison page), and the float64 reference of every sequence."""
    key = (dtype, Dh)
    if key not in _REF:
        B = len(HIST)
        lens = [None if h == OVER else h + SQ for h in HIST]
        g = torch.Generator(device=DEV).manual_seed(Dh + 17)
        q = (1.5 * torch.randn(B, SQ, H, Dh, generator=g, device=DEV)).to(dtype)
        kc = torch.full((B, BOUND + PAD, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        vc = torch.full_like(kc, float("nan"))
        pps = BOUND // PS
        need = [0 if n is None else (n + PS - 1) // PS for n in lens]
        num_pages = sum(need) + 3
        order = torch.randperm(num_pages, generator=torch.Generator().manual_seed(Dh)).tolist()
        poison = order.pop()
        kp = torch.full((num_pages, PS, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        vp = torch.full_like(kp, float("nan"))
        full = torch.full((B, pps + 2), poison, dtype=torch.int32)
        refs = []
        for b, n in enumerate(lens):
            if n is None:
                refs.append(None)
                continue
            kc[b, :n] = torch.randn(n, Hkv, Dh, generator=g, device=DEV).to(dtype)
            vc[b, :n] = (1 + 0.5 * torch.randn(n, Hkv, Dh, generator=g, device=DEV)).to(dtype)
            for i in range(need[b]):
                page = order.pop()
                full[b, i] = page
                rows = min(PS, n - i * PS)
                kp[page, :rows], vp[page, :rows] = kc[b, i * PS:i * PS + rows], vc[b, i * PS:i * PS + rows]
            refs.append(O.attention(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], None, True, stats=True))
        hist = torch.tensor(HIST, dtype=torch.int32, device=DEV)
        _REF[key] = (q, kc, vc, kp, vp, full.to(DEV)[:, :pps], hist, lens, refs)
    return _REF[key]


@pytest.mark.parametrize("dtype,Dh", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_random_ragged_batches_against_float64(dtype, Dh):
    q, kc, vc, kp, vp, table, hist, lens, refs = _ragged(dtype, Dh)
    dense = ops.attn_prefill_kvcache(q, kc, vc, hist, BOUND, SQ)
    paged = ops.attn_prefill_paged(q, kp, vp, table, hist, BOUND, SQ)
    assert torch.isfinite(dense.float()).all() and torch.equal(bits(dense), bits(paged))
    for b, n in enumerate(lens):
        if n is None:
            assert not dense[b].view(torch.int16).any()
            continue
        ref, A, qk = refs[b]
        lim = O.bound(ref, A, qk, dtype, n, Dh, Dh ** -0.5)
        err = (dense[b:b + 1].double() - ref).abs()
        print(f"{dtype} Dh {Dh} Sk {n}: max err / bound = {float((err / lim).max()):.3f}")
        assert not (err > lim).any(), (b, n, float((err / lim).max()))


@pytest.mark.parametrize("dtype,Dh", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_every_sequence_is_bit_identical_to_the_host_length_kernel_at_every_q_tile(dtype, Dh, q_tile):
    """The reference is the parent's one-pass kernel on one sequence alone; forcing the q tile keeps both calls on one tile (the plan takes B)."""
    q, kc, vc, kp, vp, table, hist, lens, _ = _ragged(dtype, Dh)
    kq, vq, ks, vs = _quant(kp, vp)
    ckq, cvq, cks, cvs = _quant(kc, vc)
    for rows in (64, 128, 256):
        q_tile(rows)
        B, H = q.shape[0], q.shape[2]
        assert ops.attn_prefill_plan(B, H, 2, Dh, SQ, BOUND)[0] == rows == ops.attn_prefill_plan(1, H, 2, Dh, SQ, lens[0])[0]
        dense = ops.attn_prefill_kvcache(q, kc, vc, hist, BOUND, SQ)
        paged = ops.attn_prefill_paged(q, kp, vp, table, hist, BOUND, SQ)
        dense8 = ops.attn_prefill_kvcache(q, ckq, cvq, hist, BOUND, SQ, k_scale=cks, v_scale=cvs)
        paged8 = ops.attn_prefill_paged(q, kq, vq, table, hist, BOUND, SQ, k_scale=ks, v_scale=vs)
        for b, n in enumerate(lens):
            if n is None:
                continue
            want = ops.flash_attn_func(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], causal=True)
            assert torch.equal(bits(dense[b:b + 1]), bits(want)), (rows, b, "dense")
            assert torch.equal(bits(paged[b:b + 1]), bits(want)), (rows, b, "paged")
            want8 = ops.attn_prefill_kv8(q[b:b + 1], ckq[b:b + 1, :n], cvq[b:b + 1, :n], cks[b:b + 1, :n], cvs[b:b + 1, :n], causal=True)
            deq = ops.flash_attn_func(q[b:b + 1], ops.kv8_dequant(ckq[b:b + 1, :n], cks[b:b + 1, :n], dtype),
                                      ops.kv8_dequant(cvq[b:b + 1, :n], cvs[b:b + 1, :n], dtype), causal=True)
            assert torch.equal(bits(want8), bits(deq))
            assert torch.equal(bits(dense8[b:b + 1]), bits(want8)), (rows, b, "dense fp8")
            assert torch.equal(bits(paged8[b:b + 1]), bits(want8)), (rows, b, "paged fp8")


def test_table_entries_behind_the_live_range_are_never_read_and_ids_are_clamped():
    dtype, Dh = torch.float16, 64
    q, kc, vc, kp, vp, table, hist, lens, _ = _ragged(dtype, Dh)
    want = ops.attn_prefill_paged(q, kp, vp, table, hist, BOUND, SQ)
    kq, vq, ks, vs = _quant(kp, vp)
    want8 = ops.attn_prefill_paged(q, kq, vq, table, hist, BOUND, SQ, k_scale=ks, v_scale=vs)
    full = torch.empty(table.shape[0], table.shape[1] + 2, dtype=torch.int32, device=DEV)
    for junk in (-1, 2 ** 31 - 1):
        full.fill_(junk)
        for b, n in enumerate(lens):
            live = 0 if n is None else (n + PS - 1) // PS
            full[b, :live] = table[b, :live]
        view = full[:, :table.shape[1]]
        assert torch.equal(bits(ops.attn_prefill_paged(q, kp, vp, view, hist, BOUND, SQ)), bits(want)), junk
        assert torch.equal(bits(ops.attn_prefill_paged(q, kq, vq, view, hist, BOUND, SQ, k_scale=ks, v_scale=vs)), bits(want8)), junk
    # ids outside the pool INSIDE the live range are clamped into it: the call returns, and the sentinel pages around the pool stay
    guard = 2
    big_k = torch.full((kp.shape[0] + 2 * guard, *kp.shape[1:]), 3.0, dtype=dtype, device=DEV)
    big_v = torch.full_like(big_k, 5.0)
    big_k[guard:-guard], big_v[guard:-guard] = kp.nan_to_num(0.0), vp.nan_to_num(0.0)
    pk, pv = big_k[guard:-guard], big_v[guard:-guard]
    bad = table.clone()
    bad[0, 0], bad[0, 1], bad[1, 2] = -5, 10 ** 9, -(2 ** 31)
    out = ops.attn_prefill_paged(q, pk, pv, bad, hist, BOUND, SQ)
    torch.cuda.synchronize()
    clamped = bad.clamp(0, kp.shape[0] - 1)
    assert torch.equal(bits(out), bits(ops.attn_prefill_paged(q, pk, pv, clamped, hist, BOUND, SQ)))
    for t, val in ((big_k, 3.0), (big_v, 5.0)):
        assert (t[:guard] == val).all() and (t[-guard:] == val).all()


def test_same_call_twice_gives_the_same_bits():
    dtype, Dh = torch.bfloat16, 128
    q, kc, vc, kp, vp, table, hist, lens, _ = _ragged(dtype, Dh)
    for fn in (lambda: ops.attn_prefill_kvcache(q, kc, vc, hist, BOUND, SQ), lambda: ops.attn_prefill_paged(q, kp, vp, table, hist, BOUND, SQ)):
        a, b = fn(), fn()
        assert torch.equal(bits(a), bits(b)) and a.any()


def test_the_split_pair_entry_still_refuses_more_than_128_rows():
    q = torch.zeros(1, 33, 8, 64, dtype=torch.float16, device=DEV)
    kc = torch.zeros(1, 128, 2, 64, dtype=torch.float16, device=DEV)
    lens = torch.full((1,), 40, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="128"):
        _engine().attn_kvcache(q, kc, kc, lens, 128, 0, 0.125, True)
    assert torch.isfinite(_engine().attn_prefill_kvcache(q, kc, kc, lens, 128, 0, 0.125, True).float()).all()


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
HID, H, HKV, DH, L = 512, 8, 2, 64, 256
W = (H + 2 * HKV) * DH
PROMPT = 96      # 96 * G = 384 rows per KV head: beyond the split pair


def _module(max_batch_size, kv_dtype=None):
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    # the projections are stand-ins (tests/test_gpu_chunk_prefill.py): x already is the qkv tensor and the output is returned as it is
    return QuantLlamaAttentionFused(HID, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=max_batch_size,
                                    kv_layout="natural", kv_dtype=kv_dtype)


def _angles():
    inv = 1.0 / (10000.0 ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(L, device=DEV).float(), inv)
    return torch.cat([f, f], -1).contiguous()


def _draw(g, B, S, dtype):
    mul = torch.cat([torch.full((H * DH,), 1.5), torch.ones(HKV * DH), torch.full((HKV * DH,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * DH), torch.ones(HKV * DH)]).to(DEV)
    return (torch.randn(B, S, W, generator=g, device=DEV) * mul + add).to(dtype)


CACHES = ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale")


def _same_caches(a, b):
    names = [n for n in CACHES if hasattr(a, n)]
    assert names and all(getattr(a, n).view(torch.uint8).any() for n in names)
    return all(torch.equal(getattr(a, n).view(torch.uint8), getattr(b, n).view(torch.uint8)) for n in names)


@pytest.mark.parametrize("ps", [64, 128])
def test_module_takes_a_prompt_in_one_call_and_leaves_the_pools_of_the_pieces(ps):
    dtype = torch.float16
    freqs = _angles()
    x = _draw(torch.Generator(device=DEV).manual_seed(5), 1, PROMPT, dtype)
    pt = PageTable(num_pages=L // ps, page_size=ps, max_batch=2, pages_per_seq=L // ps, device=DEV)
    pt.reserve(1, 1)      # slot 1 takes page 0, so that the sequence's pages are not its dense rows
    pt.reserve(0, PROMPT)
    assert pt.pages(0)[0] != 0
    whole, pieces = _module(1), _module(1)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = whole(x, pos, freqs, block_table=pt.table, page_size=ps)
    got = []
    for i in range(0, PROMPT, 32):  # 32 * G = 128: the existing split-pair route
        got.append(pieces(x[:, i:i + 32], torch.full((1,), i, dtype=torch.int32, device=DEV), freqs, block_table=pt.table, page_size=ps))
    assert out.shape == (1, PROMPT, H * DH) and torch.isfinite(out.float()).all()
    assert _same_caches(whole, pieces)
    # float64 on the stored keys and the rotated q (the store op is the parent's and leaves its q as the module's store does)
    scratch_k, scratch_v = torch.zeros_like(whole.cache_k).view(-1, ps, HKV, DH), torch.zeros_like(whole.cache_v).view(-1, ps, HKV, DH)
    xq = ops.rope_kv_store_paged(x, freqs, scratch_k, scratch_v, pt.table, pos, H, HKV)
    idx = pt.table[0].long()
    k = whole.cache_k.view(-1, ps, HKV, DH)[idx].reshape(1, -1, HKV, DH)[:, :PROMPT]
    v = whole.cache_v.view(-1, ps, HKV, DH)[idx].reshape(1, -1, HKV, DH)[:, :PROMPT]
    assert torch.equal(bits(k), bits(scratch_k[idx].reshape(1, -1, HKV, DH)[:, :PROMPT]))
    ref, A, qk = O.attention(xq, k, v, None, True, stats=True)
    lim = O.bound(ref, A, qk, dtype, PROMPT, DH, DH ** -0.5)
    for name, o in (("whole", out), ("pieces", torch.cat(got, 1))):
        err = (o.view(1, PROMPT, H, DH).double() - ref).abs()
        print(f"{name}: max err / bound = {float((err / lim).max()):.3f}")
        assert not (err > lim).any(), name


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
def test_module_prompt_with_a_tensor_position_equals_the_host_position_forward(kv_dtype, dtype):
    """Both run the one-pass kernel on one q tile (the plan sees the same B, H, Dh, Sq): bit-identical, dense and paged."""
    freqs = _angles()
    x = _draw(torch.Generator(device=DEV).manual_seed(7), 1, PROMPT, dtype)
    host, dense, paged = _module(1, kv_dtype), _module(1, kv_dtype), _module(1, kv_dtype)
    want = host(x, 0, freqs[:PROMPT])
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = dense(x, pos, freqs)
    assert torch.isfinite(got.float()).all() and torch.equal(bits(got), bits(want)) and _same_caches(dense, host)
    table = torch.arange(L // 64, dtype=torch.int32, device=DEV).flip(0)[None].contiguous()  # the pages in reverse order
    assert torch.equal(bits(paged(x, pos, freqs, block_table=table, page_size=64)), bits(want))


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.bfloat16), ("fp8", torch.float16)], ids=["T-bf16", "fp8-f16"])
def test_module_ragged_prompt_batch_equals_two_single_sequence_modules(kv_dtype, dtype, q_tile):
    """Histories 0 and 64, a 96-token chunk each, in one call -- against two single-sequence modules with int positions.  The plan takes B,
    so the q tile is forced."""
    q_tile(64)
    freqs = _angles()
    g = torch.Generator(device=DEV).manual_seed(11)
    hist = (0, 64)
    batched, singles = _module(2, kv_dtype), [_module(1, kv_dtype), _module(1, kv_dtype)]
    for i in range(0, 64, 32):  # sequence 1's history, 32 tokens a call; sequence 0 sits these calls out
        x = _draw(g, 2, 32, dtype)
        batched(x, torch.tensor([-1, i], dtype=torch.int32, device=DEV), freqs)
        singles[1](x[1:2], i, freqs[i:i + 32])
    x = _draw(g, 2, PROMPT, dtype)
    out = batched(x, torch.tensor(hist, dtype=torch.int32, device=DEV), freqs)
    assert torch.isfinite(out.float()).all()
    names = [n for n in CACHES if hasattr(batched, n)]
    for b, p in enumerate(hist):
        want = singles[b](x[b:b + 1], p, freqs[p:p + PROMPT])
        assert torch.equal(bits(out[b:b + 1]), bits(want)), b
        for n in names:
            assert torch.equal(getattr(batched, n)[b, :p + PROMPT].view(torch.uint8), getattr(singles[b], n)[0, :p + PROMPT].view(torch.uint8)), (n, b)


def test_one_graph_of_store_and_attention_follows_the_position_across_a_page_edge():
    """A 64-token chunk at G = 4 (256 rows per KV head: the one-pass route), captured once through the module and replayed three times while
    start_pos += 64 runs on the device; 128-key pages, so the third replay stores into and attends a second page."""
    ps, dtype, chunk, steps = 128, torch.bfloat16, 64, 3
    freqs = _angles()
    g = torch.Generator(device=DEV).manual_seed(13)
    m, eager = _module(1), _module(1)
    table = torch.tensor([[1, 0]], dtype=torch.int32, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = _draw(g, 1, chunk, dtype)

    def step(mod):
        return mod(x, pos, freqs, block_table=table, page_size=ps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream (it stores the chunk the first replay stores again)
        step(m)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(m)
    for t in range(steps):
        x.copy_(_draw(g, 1, chunk, dtype))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = step(eager)
        assert torch.isfinite(out.float()).all() and torch.equal(bits(out), bits(want)), t
        pos += chunk
    assert int(pos[0]) == steps * chunk > ps and _same_caches(m, eager)
