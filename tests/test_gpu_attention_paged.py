"""The paged KV cache on the GPU (awq_attn_kvcache_paged[_kv8], awq_rope_kv_store_paged_pos[_fp8]; csrc/awq_paged.hpp): the paged needle
batches of tests/attn_paged_cases.py bit for bit against their targets and against attn_kvcache on the dense gather, FP8 pools, the plan's
own chunk over several pages per split, the store against the dense store over sentinel pools, table entries that must never be read,
determinism, one captured graph across a page edge, and the module."""
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
from llm_awq_amd.paged_kv import PageTable
from tests import attn_paged_cases as P

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


def _forced(chunk, fn):
    _capi.tune(attn_splitkv_chunk=chunk)
    try:
        return fn()
    finally:
        _capi.tune(attn_splitkv_chunk=0)


# ------------------------------------------------------------------------------------------------------------------------
# needle batches: bit equality with the targets and with the dense kernel on the gather, chunks 64 and 256
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", P.CASES, ids=P.case_id)
def test_needle_batches_bit_exact_through_the_table(spec):
    pb = P.PagedBatch(spec)
    batch = pb.batch
    q, lens, kp, vp = (t.to(DEV) for t in (batch.q, batch.seqlens_k, pb.k_pool, pb.v_pool))
    table = pb.table_full.to(DEV)[:, :pb.pps]  # the row stride stays wider than pages_per_seq
    assert table.stride(0) == pb.pps + P.PAD_COLS
    kd, vd = (t.to(DEV) for t in pb.dense())
    scale = q.shape[3] ** -0.5 if batch.scale is None else batch.scale
    for chunk in P.CHUNKS:
        def run():
            out = ops.attn_kvcache_paged(q, kp, vp, table, lens, batch.bound, batch.offset, batch.scale, batch.causal)
            eng = _engine().attn_kvcache_paged(q, kp, vp, table, lens, batch.bound, batch.offset, scale, batch.causal)
            dense = ops.attn_kvcache(q, kd, vd, lens, batch.bound, batch.offset, batch.scale, batch.causal)
            return out, eng, dense
        out, eng, dense = _forced(chunk, run)
        torch.cuda.synchronize()
        assert out.shape == batch.target.shape and out.is_contiguous()
        _assert_bits(out, batch.target, ("target", chunk))
        _assert_bits(eng, batch.target, ("engine", chunk))
        _assert_bits(out, dense, ("dense gather", chunk))
        for b, n in enumerate(batch.lens):
            if n is None:
                assert not out[b].view(torch.int16).any()  # exactly zero, not -0


# ------------------------------------------------------------------------------------------------------------------------
# random ragged batches on a shuffled pool (shared by the tests below, never written to)
# ------------------------------------------------------------------------------------------------------------------------
_POOL = {}


def _random_pool(dtype, Dh, lens, ps, pps, Sq=1, H=8, Hkv=2, poison=True):
    """q, pools whose unused rows are NaN, a shuffled table (entries behind the live range: the NaN poison page), the lengths and the dense
    gather [B, pps * ps, Hkv, Dh]."""
    key = (dtype, Dh, lens, ps, pps, Sq)
    if key not in _POOL:
        B = len(lens)
        g = torch.Generator(device=DEV).manual_seed(Dh + sum(n or 0 for n in lens) + ps)
        need = [0 if n is None else (n + ps - 1) // ps for n in lens]
        num_pages = sum(need) + 3
        order = torch.randperm(num_pages, generator=torch.Generator().manual_seed(ps + Dh)).tolist()
        poison_page = order.pop()
        q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dtype)
        kp = torch.full((num_pages, ps, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        vp = torch.full((num_pages, ps, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        full = torch.full((B, pps + 2), poison_page, dtype=torch.int32)
        for b, n in enumerate(lens):
            for i in range(need[b]):
                page = order.pop()
                full[b, i] = page
                rows = min(ps, n - i * ps)
                kp[page, :rows] = torch.randn(rows, Hkv, Dh, generator=g, device=DEV).to(dtype)
                vp[page, :rows] = (1 + 0.5 * torch.randn(rows, Hkv, Dh, generator=g, device=DEV)).to(dtype)
        table = full.to(DEV)[:, :pps]
        idx = table.long()
        kd, vd = (t[idx].reshape(B, pps * ps, Hkv, Dh) for t in (kp, vp))
        dl = torch.tensor([-1 if n is None else n for n in lens], dtype=torch.int32, device=DEV)
        _POOL[key] = (q, kp, vp, table, dl, kd, vd)
    return _POOL[key]


PLAN_LENS, PLAN_BOUND, PLAN_PS = (2049, 1025, 300, None), 2304, 256


def test_the_plans_own_chunk_walks_several_pages_per_split():
    """Page size 256, bound 2304: the unforced plan is 3 splits of 1024 keys, four pages each; 2049 keys end one key into the third."""
    dtype, Dh = torch.bfloat16, 128
    q, kp, vp, table, lens, kd, vd = _random_pool(dtype, Dh, PLAN_LENS, PLAN_PS, PLAN_BOUND // PLAN_PS)
    assert ops.attn_kvcache_plan(len(PLAN_LENS), 8, 2, Dh, 1, PLAN_BOUND) == (3, 1024)
    out = ops.attn_kvcache_paged(q, kp, vp, table, lens, PLAN_BOUND)
    dense = ops.attn_kvcache(q, kd, vd, lens, PLAN_BOUND)
    assert torch.isfinite(out.float()).all() and out[:3].any() and not out[3].view(torch.int16).any()
    assert torch.equal(bits(out), bits(dense))
    # the lengths before the step and seqlen_offset = 1, as a decode step passes them
    assert torch.equal(bits(ops.attn_kvcache_paged(q, kp, vp, table, lens - 1, PLAN_BOUND, 1)), bits(out))


@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_fp8_pools_equal_the_t_form_on_the_dequantised_pools(dtype, Dh):
    """A needle batch (forced chunk 64) and the random ragged batch (the plan's chunk), paged FP8 against paged T on the dequantised pools,
    and against the dense FP8 entry on the gather of codes and scales."""
    spec = next(s for s in P.CASES if s["Sq"] == 8 and s["mode"] == "scatter" and s["dtype"] == dtype and s["page_size"] == 128)
    pb = P.PagedBatch(spec)
    batch = pb.batch
    needle = (batch.q.to(DEV), pb.k_pool.to(DEV), pb.v_pool.to(DEV), pb.table_full.to(DEV)[:, :pb.pps], batch.seqlens_k.to(DEV), batch.bound,
              batch.offset, 64)
    q, kp, vp, table, lens, _, _ = _random_pool(dtype, Dh, PLAN_LENS, PLAN_PS, PLAN_BOUND // PLAN_PS)
    for q, kp, vp, table, lens, bound, offset, chunk in (needle, (q, kp, vp, table, lens, PLAN_BOUND, 0, 0)):
        kp, vp = kp.nan_to_num(0.0), vp.nan_to_num(0.0)  # (a NaN row has no scale; nothing behind a live range is read anyway)
        kq, ks = ops.kv8_quant(kp)
        vq, vs = ops.kv8_quant(vp)

        def run():
            got = ops.attn_kvcache_paged(q, kq, vq, table, lens, bound, offset, None, True, k_scale=ks, v_scale=vs)
            want = ops.attn_kvcache_paged(q, ops.kv8_dequant(kq, ks, dtype), ops.kv8_dequant(vq, vs, dtype), table, lens, bound, offset, None, True)
            eng = _engine().attn_kvcache_paged_kv8(q, kq, vq, ks, vs, table, lens, bound, offset, q.shape[3] ** -0.5, True)
            idx = table.long()
            B, n = idx.shape[0], idx.shape[1] * kq.shape[1]
            dense = ops.attn_kvcache(q, kq[idx].reshape(B, n, *kq.shape[2:]), vq[idx].reshape(B, n, *vq.shape[2:]), lens, bound, offset, None, True,
                                     k_scale=ks[idx].reshape(B, n, -1), v_scale=vs[idx].reshape(B, n, -1))
            return got, want, eng, dense
        got, want, eng, dense = _forced(chunk, run)
        assert torch.isfinite(got.float()).all() and got.any()
        assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got), bits(eng)) and torch.equal(bits(got), bits(dense))


def test_entries_behind_the_live_range_are_never_read():
    """-1 and 2**31 - 1 behind every sequence's last page, and in the whole row of the inactive sequence: the results do not change."""
    dtype, Dh = torch.float16, 64
    q, kp, vp, table, lens, kd, vd = _random_pool(dtype, Dh, PLAN_LENS, PLAN_PS, PLAN_BOUND // PLAN_PS)
    want = ops.attn_kvcache_paged(q, kp, vp, table, lens, PLAN_BOUND)
    full = torch.empty(table.shape[0], table.shape[1] + 2, dtype=torch.int32, device=DEV)
    for junk in (-1, 2 ** 31 - 1):
        full.fill_(junk)
        for b, n in enumerate(PLAN_LENS):
            live = 0 if n is None else (n + PLAN_PS - 1) // PLAN_PS
            full[b, :live] = table[b, :live]
        got = ops.attn_kvcache_paged(q, kp, vp, full[:, :table.shape[1]], lens, PLAN_BOUND)
        assert torch.equal(bits(got), bits(want)), junk
        kq, ks = ops.kv8_quant(kp.nan_to_num(0.0))
        vq, vs = ops.kv8_quant(vp.nan_to_num(0.0))
        a = ops.attn_kvcache_paged(q, kq, vq, full[:, :table.shape[1]], lens, PLAN_BOUND, k_scale=ks, v_scale=vs)
        b_ = ops.attn_kvcache_paged(q, kq, vq, table, lens, PLAN_BOUND, k_scale=ks, v_scale=vs)
        assert torch.equal(bits(a), bits(b_)), junk


def test_same_call_twice_gives_the_same_bits_and_a_nan_workspace_changes_nothing():
    dtype, Dh = torch.float16, 64
    q, kp, vp, table, lens, _, _ = _random_pool(dtype, Dh, PLAN_LENS, PLAN_PS, PLAN_BOUND // PLAN_PS)
    a = ops.attn_kvcache_paged(q, kp, vp, table, lens, PLAN_BOUND)
    b = ops.attn_kvcache_paged(q, kp, vp, table, lens, PLAN_BOUND)
    assert torch.equal(bits(a), bits(b))
    B, Sq, H, _ = q.shape
    L = _capi.lib()
    wsb = L.awq_attn_kvcache_workspace_bytes(B, H, 2, Dh, Sq, PLAN_BOUND)
    ws = torch.full((wsb // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full_like(a, float("nan"))
    with torch.cuda.device(q.device):
        _capi.check(L.awq_attn_kvcache_paged(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), out.data_ptr(), table.data_ptr(), B, Sq, lens.data_ptr(), 0,
                                             PLAN_BOUND, kp.shape[0], kp.shape[1], table.shape[1], table.stride(0), H, 2, Dh, q.stride(0), q.stride(1),
                                             kp.stride(0), kp.stride(1), vp.stride(0), vp.stride(1), Dh ** -0.5, 1, 0, ws.data_ptr(), wsb,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(a))


# ------------------------------------------------------------------------------------------------------------------------
# the store
# ------------------------------------------------------------------------------------------------------------------------
H, HKV = 8, 2
STORE_POS = {1: (0, 63, 64, 130, -1, 10 ** 6), 5: (62, 126, 0, 60, -1, None)}  # None: four keys before the end of the table row, one too few


def _sentinel(shape, dtype, mul):
    n = 1
    for d in shape:
        n *= d
    pat = (torch.arange(n, device=DEV) * mul + 12345) % 30011  # as 16-bit patterns: finite and positive
    if dtype == torch.uint8:
        return (pat % 251).to(torch.uint8).reshape(shape).clone()
    if dtype == torch.float32:
        return (pat.float() + 0.5).reshape(shape).clone()
    return pat.to(torch.int16).view(dtype).reshape(shape).clone()


def _store_setup(S, ps, Dh, dtype):
    L = 320
    pps = (L + ps - 1) // ps
    pos = tuple(pps * ps - 4 if p is None else p for p in STORE_POS[S])
    B = len(pos)
    g = torch.Generator().manual_seed(S + ps + Dh)
    num_pages = B * pps + 2
    perm = torch.randperm(num_pages, generator=g)
    full = torch.full((B, pps + 3), int(perm[-1]), dtype=torch.int32)
    full[:, :pps] = perm[:B * pps].reshape(B, pps).int()
    table = full.to(DEV)[:, :pps]
    gd = torch.Generator(device=DEV).manual_seed(S * 7 + Dh)
    qkv = torch.randn(B, S, (H + 2 * HKV) * Dh, generator=gd, device=DEV).to(dtype)
    freqs = (50.0 * torch.randn(pps * ps + 20, Dh // 2 if S == 1 else Dh, generator=gd, device=DEV)).contiguous()
    lens = torch.tensor(pos, dtype=torch.int32, device=DEV)
    return pos, B, pps, num_pages, table, qkv, freqs, lens


@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128)], ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("ps", P.PAGE_SIZES)
@pytest.mark.parametrize("S", [1, 5])
def test_store_leaves_the_dense_stores_bits_in_the_rows_the_table_names_and_nothing_else(S, ps, dtype, Dh):
    E = _engine()
    pos, B, pps, num_pages, table, qkv, freqs, lens = _store_setup(S, ps, Dh, dtype)
    idx = table.long()
    kp0, vp0 = _sentinel((num_pages, ps, HKV, Dh), dtype, 7), _sentinel((num_pages, ps, HKV, Dh), dtype, 13)
    # the dense store on the gather of the sentinel pools, scattered back: what the pools must hold, every byte
    kd, vd = (t[idx].reshape(B, pps * ps, HKV, Dh).contiguous() for t in (kp0, vp0))
    q_want = ops.rope_kv_store_natural_pos(qkv, freqs, kd, vd, lens, H, HKV)
    kp_want, vp_want = kp0.clone(), vp0.clone()
    kp_want[idx] = kd.reshape(B, pps, ps, HKV, Dh)
    vp_want[idx] = vd.reshape(B, pps, ps, HKV, Dh)
    assert not torch.equal(bits(kp_want), bits(kp0)) and not q_want[4:].view(torch.int16).any() and q_want[:4].any()
    for fn in (ops.rope_kv_store_paged, E.rope_kv_store_paged_pos):
        kp, vp = kp0.clone(), vp0.clone()
        q_out = fn(qkv, freqs, kp, vp, table, lens, H, HKV)
        torch.cuda.synchronize()
        assert q_out.shape == (B, S, H, Dh) and torch.equal(bits(q_out), bits(q_want))
        assert torch.equal(bits(kp), bits(kp_want)) and torch.equal(bits(vp), bits(vp_want))  # the WHOLE pools
    # FP8: codes and scales
    zero = (_sentinel((num_pages, ps, HKV, Dh), torch.uint8, 7), _sentinel((num_pages, ps, HKV, Dh), torch.uint8, 13),
            _sentinel((num_pages, ps, HKV), torch.float32, 3), _sentinel((num_pages, ps, HKV), torch.float32, 5))
    dense = [t[idx].reshape(B, pps * ps, *t.shape[2:]).contiguous() for t in zero]
    q8 = ops.rope_kv_store_natural_pos(qkv, freqs, dense[0], dense[1], lens, H, HKV, k_scale=dense[2], v_scale=dense[3])
    assert torch.equal(bits(q8), bits(q_want))
    want = [t.clone() for t in zero]
    for w, d in zip(want, dense):
        w[idx] = d.reshape(B, pps, ps, *d.shape[2:])
    for fn in (lambda *a: ops.rope_kv_store_paged(*a[:4], a[6], a[7], a[8], a[9], k_scale=a[4], v_scale=a[5]), E.rope_kv_store_paged_pos_fp8):
        got = [t.clone() for t in zero]
        q_out = fn(qkv, freqs, *got, table, lens, H, HKV)
        torch.cuda.synchronize()
        assert torch.equal(bits(q_out), bits(q_want))
        for g_, w in zip(got, want):
            assert torch.equal(g_.view(torch.uint8), w.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------------
# the module: equal to the dense device-position forward, and one captured graph across a page edge
# ------------------------------------------------------------------------------------------------------------------------
HID, DH, L = 512, 64, 256
W = (H + 2 * HKV) * DH


def _module(max_batch_size, kv_dtype=None):
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
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


def _history(mods, g, lens, dtype, freqs, table=None, ps=None, piece=16):
    """The same `lens[b]` tokens (multiples of `piece`) through every module, B-wide: a sequence whose history is complete sits the call
    out with position -1."""
    B = len(lens)
    for i in range(0, max(lens), piece):
        x = _draw(g, B, piece, dtype)
        pos = torch.tensor([i if i < n else -1 for n in lens], dtype=torch.int32, device=DEV)
        for m in mods:
            kw = dict(block_table=table, page_size=ps) if getattr(m, "paged_test", False) else {}
            m(x, pos, freqs, **kw)


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
def test_module_with_a_block_table_equals_the_dense_device_position_forward(kv_dtype, dtype):
    ps, B = 64, 3
    freqs = _angles()
    g = torch.Generator(device=DEV).manual_seed(23)
    paged, dense = _module(B, kv_dtype), _module(B, kv_dtype)
    paged.paged_test = True
    names = [n for n in CACHES if hasattr(paged, n)]
    assert len(names) == (4 if kv_dtype else 2)
    pt = PageTable(num_pages=B * L // ps, page_size=ps, max_batch=B, pages_per_seq=L // ps, device=DEV)
    cur = [48, 16, 96]
    for b in (2, 0, 1):  # slot 2 takes page 0 first, so that no slot's pages are its dense rows
        pt.reserve(b, cur[b])
    assert pt.pages(0)[0] != 0 and pt.pages(1)[0] != L // ps
    ptrs = [getattr(paged, n).data_ptr() for n in names] + [pt.table.data_ptr()]

    def run():
        _history((paged, dense), g, cur, dtype, freqs, pt.table, ps)
        pos = torch.tensor(cur, dtype=torch.int32, device=DEV)
        for step, S in enumerate((13, 5, 1, 1, 1)):  # two prompt pieces (the second takes sequence 0 over key 64, a new page), then decode
            for b in range(B):
                pt.reserve(b, cur[b] + S)
            x = _draw(g, B, S, dtype)
            got = paged(x, pos, freqs, block_table=pt.table, page_size=ps)
            want = dense(x, pos, freqs)
            assert got.shape == (B, S, H * DH) and torch.isfinite(got.float()).all() and got.any()
            assert torch.equal(bits(got), bits(want)), step
            pos += S
            for b in range(B):
                cur[b] += S
        # a finished slot: nothing is stored for it, its rows are zeros
        x = _draw(g, B, 1, dtype)
        before = [getattr(paged, n).clone() for n in names]
        off = torch.tensor([cur[0], -1, cur[2]], dtype=torch.int32, device=DEV)
        pt.reserve(0, cur[0] + 1), pt.reserve(2, cur[2] + 1)
        got = paged(x, off, freqs, block_table=pt.table, page_size=ps)
        assert not got[1].view(torch.int16).any() and torch.equal(bits(got), bits(dense(x, off, freqs)))
        idx = pt.table.long()
        for n, old in zip(names, before):  # sequence 1's pages did not change
            pool, was = getattr(paged, n), old
            pool, was = pool.view(-1, ps, *pool.shape[2:]), was.view(-1, ps, *was.shape[2:])
            mine = idx[1, :len(pt.pages(1))]
            assert torch.equal(pool[mine].view(torch.uint8), was[mine].view(torch.uint8))
    _forced(64, run)  # several splits per sequence
    assert [getattr(paged, n).data_ptr() for n in names] + [pt.table.data_ptr()] == ptrs  # nothing was copied or allocated
    idx = pt.table.long()
    for n in names:  # the pool rows the table names hold the dense caches' bytes
        pool = getattr(paged, n)
        pool = pool.view(-1, ps, *pool.shape[2:])
        gathered = pool[idx].reshape(B, L, *pool.shape[2:])
        for b in range(B):
            assert torch.equal(gathered[b, :cur[b]].view(torch.uint8), getattr(dense, n)[b, :cur[b]].view(torch.uint8)), (n, b)
            assert getattr(dense, n)[b, :cur[b]].view(torch.uint8).any()
    with pytest.raises(ValueError, match="start_pos"):
        paged(torch.zeros(B, 1, W, dtype=dtype, device=DEV), 3, freqs, block_table=pt.table, page_size=ps)


def test_one_graph_follows_the_positions_and_the_table_across_a_page_edge():
    """Store + attention through the module, captured once: the replays follow start_pos += 1 on the device and an in-place table update
    when sequence 0 reaches key 64, a new page.  Bit-equal to the eager calls of a second module that shares the table."""
    ps, B, dtype, steps = 64, 2, torch.bfloat16, 5
    freqs = _angles()
    g = torch.Generator(device=DEV).manual_seed(29)
    m, eager = _module(B), _module(B)
    m.paged_test = eager.paged_test = True
    pt = PageTable(num_pages=B * L // ps, page_size=ps, max_batch=B, pages_per_seq=L // ps, device=DEV)
    start = [48, 128]
    for b in (1, 0):
        pt.reserve(b, start[b])
    _capi.tune(attn_splitkv_chunk=64)
    try:
        _history((m, eager), g, start, dtype, freqs, pt.table, ps)
        x14 = _draw(g, B, 14, dtype)  # sequence 0 to 62 keys, sequence 1 to 142
        for b in range(B):
            pt.reserve(b, start[b] + 14)
        pos = torch.tensor(start, dtype=torch.int32, device=DEV)
        for mod in (m, eager):
            mod(x14, pos, freqs, block_table=pt.table, page_size=ps)
        pos += 14
        start = [n + 14 for n in start]
        assert start[0] == 62 and len(pt.pages(0)) == 1
        x = _draw(g, B, 1, dtype)

        def step(mod):
            return mod(x, pos, freqs, block_table=pt.table, page_size=ps)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream (it stores the token the first replay stores again)
            step(m)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step(m)
        table_ptr = pt.table.data_ptr()
        for t in range(steps):
            for b in range(B):
                pt.reserve(b, start[b] + t + 1)  # in place, between replays
            x.copy_(_draw(g, B, 1, dtype))
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            want = step(eager)
            assert torch.isfinite(out.float()).all() and torch.equal(bits(out), bits(want)), t
            pos += 1
        assert len(pt.pages(0)) == 2 and start[0] + steps > 64 and pt.table.data_ptr() == table_ptr  # the table grew under the graph
        assert torch.equal(bits(m.cache_k), bits(eager.cache_k)) and torch.equal(bits(m.cache_v), bits(eager.cache_v)) and m.cache_k.any()
    finally:
        _capi.tune(attn_splitkv_chunk=0)
