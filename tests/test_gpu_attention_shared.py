"""Shared-prefix decode on the GPU (awq_attn_kvcache_paged_shared[_kv8], awq_kv_page_copy[_fp8]; csrc/awq_shared.hpp): the needle batches of
tests/attn_shared_cases.py bit for bit against their targets and against attn_kvcache_paged on the same pools and tables, FP8 pools, the
plan's own chunk, a prefix that is no multiple of the chunk against float64, table entries that must never be read, a lead that leaves
under one captured graph, a NaN workspace, the page copy over sentinel pools, and the module."""
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
from llm_awq_amd.paged_kv import PageTable, PrefixGroups
from tests import attn_prefill_oracle as O
from tests import attn_shared_cases as C
from tests import attn_splitkv_oracle as S

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


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------
# needle batches: bit equality with the targets and with attn_kvcache_paged, chunks 64 and 256, T and FP8, ops and engine
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_needle_batches_bit_exact(spec):
    sb = C.build(spec)
    q, lens, kp, vp = (t.to(DEV) for t in (sb.q, sb.seqlens_k, sb.k_pool, sb.v_pool))
    table = sb.table_full.to(DEV)[:, :sb.pps]  # the row stride stays wider than pages_per_seq
    poisoned = sb.poisoned_table().to(DEV)[:, :sb.pps]
    assert table.stride(0) == sb.pps + C.PAD_COLS
    gm_full = torch.full((len(sb.members), sb.cap + 2), -1, dtype=torch.int32)
    gm_full[:, :sb.cap] = torch.tensor(sb.members, dtype=torch.int32)
    gm = gm_full.to(DEV)[:, :sb.cap]                 # a row stride of its own
    gp, sp = _i32(sb.group_prefix), _i32(sb.seq_prefix)
    scale = q.shape[3] ** -0.5
    kq, ks = ops.kv8_quant(kp.nan_to_num(0.0))       # (a NaN row has no scale; nothing behind a live range is read anyway)
    vq, vs = ops.kv8_quant(vp.nan_to_num(0.0))
    kd, vd = ops.kv8_dequant(kq, ks, q.dtype), ops.kv8_dequant(vq, vs, q.dtype)
    E = _engine()
    for chunk in C.CHUNKS:
        def run():
            args = (lens, sb.bound, gm, gp, sp, sb.max_prefix, sb.offset)
            return dict(ops=ops.attn_kvcache_paged_shared(q, kp, vp, table, *args),
                        eng=E.attn_kvcache_paged_shared(q, kp, vp, table, *args, scale, True),
                        poison=ops.attn_kvcache_paged_shared(q, kp, vp, poisoned, *args),
                        paged=ops.attn_kvcache_paged(q, kp, vp, table, lens, sb.bound, sb.offset),
                        f8=ops.attn_kvcache_paged_shared(q, kq, vq, table, *args, k_scale=ks, v_scale=vs),
                        f8eng=E.attn_kvcache_paged_shared_kv8(q, kq, vq, ks, vs, table, *args, scale, True),
                        f8t=ops.attn_kvcache_paged_shared(q, kd, vd, table, *args),
                        f8paged=ops.attn_kvcache_paged(q, kq, vq, table, lens, sb.bound, sb.offset, k_scale=ks, v_scale=vs))
        r = _forced(chunk, run)
        torch.cuda.synchronize()
        ok = sb.defined(chunk).to(DEV)
        assert ok.any() and r["ops"].shape == sb.target.shape and r["ops"].is_contiguous()
        want = sb.target.to(DEV)[ok]
        for name in ("ops", "eng", "poison"):
            _assert_bits(r[name][ok], want, (name, chunk))
        for b, n in enumerate(sb.lens_spec):
            if n is None:
                assert not r["ops"][b].view(torch.int16).any()  # exactly zero, not -0
        _assert_bits(r["f8"][ok], r["f8t"][ok], ("fp8 against T on the dequantised pools", chunk))
        _assert_bits(r["f8eng"][ok], r["f8"][ok], ("fp8 engine", chunk))
        if C.P % chunk == 0:  # the contract's bit identity with the unshared call
            _assert_bits(r["ops"][ok], r["paged"][ok], ("attn_kvcache_paged", chunk))
            _assert_bits(r["f8"][ok], r["f8paged"][ok], ("attn_kvcache_paged_kv8", chunk))


# ------------------------------------------------------------------------------------------------------------------------
# random data: sequences that share a prefix on a shuffled pool whose page 0 is NaN (built once per shape, never written to)
# ------------------------------------------------------------------------------------------------------------------------
_POOL = {}


def _shared_pool(dtype, Dh, P, owns, ps, pps, Sq=1, H=8, Hkv=2, extra=()):
    """len(owns) members of one group share P keys (P % ps == 0: the same page ids) and bring owns[j] keys of their own; `extra` are the
    lengths of ungrouped slots behind them.  Unused pool rows and pages 0 and 1 are NaN; table entries behind a live range name page 1."""
    key = (dtype, Dh, P, owns, ps, pps, Sq, extra)
    if key not in _POOL:
        assert P % ps == 0
        lens = [P + o for o in owns] + list(extra)
        B = len(lens)
        g = torch.Generator(device=DEV).manual_seed(Dh + sum(lens) + ps + Sq)
        need = [(n + ps - 1) // ps for n in lens]
        num_pages = P // ps + sum(need) + 2
        order = [p for p in torch.randperm(num_pages, generator=torch.Generator().manual_seed(ps + Dh)).tolist() if p > 1]
        q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dtype)
        kp = torch.full((num_pages, ps, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        vp = torch.full((num_pages, ps, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
        full = torch.full((B, pps + 2), 1, dtype=torch.int32)
        prefix_pages = [order.pop() for _ in range(P // ps)]
        for b, n in enumerate(lens):
            mine = list(prefix_pages) if b < len(owns) else []
            for i in range(need[b]):
                fresh = i >= len(mine)
                page = order.pop() if fresh else mine[i]
                full[b, i] = page
                rows = min(ps, n - i * ps)
                if fresh or b == 0:
                    kp[page, :rows] = torch.randn(rows, Hkv, Dh, generator=g, device=DEV).to(dtype)
                    vp[page, :rows] = (1 + 0.5 * torch.randn(rows, Hkv, Dh, generator=g, device=DEV)).to(dtype)
        table = full.to(DEV)[:, :pps]
        gm = _i32([list(range(len(owns)))])
        sp = _i32([P] * len(owns) + [0] * len(extra))
        _POOL[key] = (q, kp, vp, table, _i32(lens), gm, _i32([P]), sp, lens)
    return _POOL[key]


def _gather(kp, vp, table, b, n):
    p = torch.arange(n, device=DEV)
    page = table[b, p // kp.shape[1]].long()
    return kp[page, p % kp.shape[1]][None], vp[page, p % kp.shape[1]][None]


PLAN = dict(dtype=torch.bfloat16, Dh=128, P=2048, owns=(256, 1, 130, 77), ps=256, pps=9, extra=(300,))


def test_the_plans_own_chunk_equals_the_unshared_call():
    """max_prefix 2048 under the bound 2304: both plans choose 1024-key chunks, the prefix is two of them, and the bits are attn_kvcache_paged's."""
    q, kp, vp, table, lens, gm, gp, sp, _ = _shared_pool(**PLAN)
    assert ops.attn_kvcache_shared_plan(q.shape[0], 8, 2, 128, 1, 2048, 2304) == (2, 1024, 3, 1024)
    out = ops.attn_kvcache_paged_shared(q, kp, vp, table, lens, 2304, gm, gp, sp, 2048)
    want = ops.attn_kvcache_paged(q, kp, vp, table, lens, 2304)
    assert torch.isfinite(out.float()).all() and out.any()
    assert torch.equal(bits(out), bits(want))
    # the lengths before the step and seqlen_offset = 1, as a decode step passes them; and the engine
    assert torch.equal(bits(ops.attn_kvcache_paged_shared(q, kp, vp, table, lens - 1, 2304, gm, gp, sp, 2048, 1)), bits(out))
    assert torch.equal(bits(_engine().attn_kvcache_paged_shared(q, kp, vp, table, lens, 2304, gm, gp, sp, 2048, 0, 128 ** -0.5, True)), bits(out))


def _check(out, ref, lim, what):
    assert torch.isfinite(out.float()).all(), what
    err = (out.double() - ref).abs()
    print(f"{what}: max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (what, int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("dtype,Dh,Sq", [(torch.float16, 64, 1), (torch.bfloat16, 128, 3), (torch.float16, 128, 3), (torch.bfloat16, 64, 1)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_a_prefix_that_is_no_multiple_of_the_chunk_stays_within_the_bound(dtype, Dh, Sq):
    """P = 192 under a forced chunk of 128: prefix splits [0, 128) and [128, 192), suffix splits from 192 -- other cuts than the unshared
    call's, so no bit identity; every row of every slot within tests.attn_splitkv_oracle.bound of float64, `splits` = all entries a row combines."""
    q, kp, vp, table, lens, gm, gp, sp, host_lens = _shared_pool(dtype, Dh, 192, (Sq, 70, 130), 64, 6, Sq=Sq, extra=(150,))
    bound, max_prefix = 384, 256
    out = _forced(128, lambda: ops.attn_kvcache_paged_shared(q, kp, vp, table, lens, bound, gm, gp, sp, max_prefix))
    splits = max_prefix // 128 + bound // 128
    for b, n in enumerate(host_lens):
        k, v = _gather(kp, vp, table, b, n)
        ref, Aw, qk = O.attention(q[b:b + 1], k, v, None, True, stats=True)
        _check(out[b:b + 1], ref, S.bound(ref, Aw, qk, dtype, n, Dh, Dh ** -0.5, splits), f"slot {b} ({n} keys)")


def test_a_nan_workspace_changes_nothing_twice_over():
    q, kp, vp, table, lens, gm, gp, sp, _ = _shared_pool(**PLAN)
    want = ops.attn_kvcache_paged_shared(q, kp, vp, table, lens, 2304, gm, gp, sp, 2048)
    B, Sq, H, Dh = q.shape
    L = _capi.lib()
    wsb = L.awq_attn_kvcache_shared_workspace_bytes(B, H, 2, Dh, Sq, 2048, 2304)
    assert wsb == B * H * Sq * 5 * (Dh + 2) * 4
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=DEV)
    for _ in range(2):
        ws.fill_(float("nan"))
        out = torch.full_like(want, float("nan"))
        with torch.cuda.device(q.device):
            _capi.check(L.awq_attn_kvcache_paged_shared(
                q.data_ptr(), kp.data_ptr(), vp.data_ptr(), out.data_ptr(), table.data_ptr(), B, Sq, lens.data_ptr(), 0, 2304, kp.shape[0],
                kp.shape[1], table.shape[1], table.stride(0), H, 2, Dh, q.stride(0), q.stride(1), kp.stride(0), kp.stride(1), vp.stride(0),
                vp.stride(1), Dh ** -0.5, 1, 1, gm.data_ptr(), gp.data_ptr(), sp.data_ptr(), 1, gm.shape[1], gm.stride(0), 2048, ws.data_ptr(),
                wsb, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want))


def test_one_graph_follows_a_lead_that_leaves():
    """The group's lead turns inactive in place (length -1, its table row zeroed: page 0 holds NaN) between two replays of one graph: the
    next listed member leads, and the remaining members keep their bits."""
    q, kp, vp, table, lens, gm, gp, sp, _ = _shared_pool(torch.float16, 64, 192, (1, 70, 130, 40), 64, 6, extra=(150,))
    lens, table = lens.clone(), table.clone()
    assert torch.isnan(kp[0]).all()

    def step():
        return ops.attn_kvcache_paged_shared(q, kp, vp, table, lens, 384, gm, gp, sp, 256)
    _capi.tune(attn_splitkv_chunk=64)
    try:
        want = ops.attn_kvcache_paged(q, kp, vp, table, lens, 384)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want)) and out.any()
        lens[0:1].fill_(-1)
        table[0].zero_()
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert not out[0].view(torch.int16).any() and torch.equal(bits(out[1:]), bits(want[1:]))
    finally:
        _capi.tune(attn_splitkv_chunk=0)


# ------------------------------------------------------------------------------------------------------------------------
# kv_page_copy
# ------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("Dh,ps", [(64, 64), (128, 192)])
def test_page_copy_moves_the_named_pages_and_nothing_else(fp8, Dh, ps):
    """Pools that are strided views (padding between rows and between pages), 7 pairs of which one has equal ids and three an id outside
    the pool: the named pages hold the source's bytes, every other byte -- the padding included -- is what it was."""
    num_pages, Hkv = 9, 3
    dt = torch.uint8 if fp8 else torch.bfloat16
    backing = [_sentinel((num_pages, ps + 1, Hkv + 1, Dh), dt, m) for m in (7, 13)]
    pools = [torch.as_strided(b, (num_pages, ps, Hkv, Dh), (b.stride(0), b.stride(1), Dh, 1)) for b in backing]  # heads contiguous, rows padded
    sback = [_sentinel((num_pages, ps + 2, Hkv + 3), torch.float32, m) for m in (3, 5)] if fp8 else []
    scales = [b[:, :ps, :Hkv] for b in sback]
    src = _i32([2, 5, 4, -1, 3, num_pages, 0])
    dst = _i32([7, 1, 4, 6, num_pages, 8, -2])
    moved = {7: 2, 1: 5}
    E = _engine()
    for fn in ("ops", "eng"):
        got_b = [b.clone() for b in backing + sback]
        got = [torch.as_strided(g, p.shape, p.stride()) for g, p in zip(got_b, pools + scales)]
        if fn == "ops":
            ops.kv_page_copy(got[0], got[1], src, dst, *got[2:])
        elif fp8:
            E.kv_page_copy_fp8(*got, src, dst)
        else:
            E.kv_page_copy(*got, src, dst)
        torch.cuda.synchronize()
        for g, was_b, was in zip(got_b, backing + sback, pools + scales):
            want_b = was_b.clone()
            want = torch.as_strided(want_b, was.shape, was.stride())
            for d, s_ in moved.items():
                want[d] = was[s_]
            assert torch.equal(g.view(torch.uint8), want_b.view(torch.uint8)), fn
            assert not torch.equal(g.view(torch.uint8), was_b.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------------
# the module: a prompt, three forks and four decode steps equal the unshared paged forward
# ------------------------------------------------------------------------------------------------------------------------
H, HKV, HID, DH, L = 8, 2, 512, 64, 384
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


def _draw(g, B, S_, dtype):
    mul = torch.cat([torch.full((H * DH,), 1.5), torch.ones(HKV * DH), torch.full((HKV * DH,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * DH), torch.ones(HKV * DH)]).to(DEV)
    return (torch.randn(B, S_, W, generator=g, device=DEV) * mul + add).to(dtype)


@pytest.mark.parametrize("kv_dtype,dtype,ps", [(None, torch.float16, 64), ("fp8", torch.bfloat16, 128)], ids=["T-f16-ps64", "fp8-bf16-ps128"])
def test_module_with_forks_and_prefix_groups_equals_the_unshared_paged_forward(kv_dtype, dtype, ps):
    """Page size 64: the 320-token prompt is five whole pages, all shared.  Page size 128: two shared pages and a 64-token tail that
    `fork` has copied with kv_page_copy; the group then shares the 256 tokens of the whole pages."""
    B, prompt, piece = 4, 320, 64
    freqs = _angles()
    g = torch.Generator(device=DEV).manual_seed(31)
    shared, plain = _module(B, kv_dtype), _module(B, kv_dtype)
    tables = [PageTable(num_pages=B * L // ps, page_size=ps, max_batch=B, pages_per_seq=L // ps, device=DEV) for _ in range(2)]
    st, pt = tables
    pt.reserve(3, ps)  # the unshared slots do not get the shared module's page ids
    st.reserve(0, prompt)
    for b in range(B):
        pt.reserve(b, prompt)

    def run():
        for i in range(0, prompt, piece):  # the prompt: once into the shared module, once per slot into the unshared one
            x = _draw(g, 1, piece, dtype).expand(B, piece, W).contiguous()
            shared(x, _i32([i, -1, -1, -1]), freqs, block_table=st.table, page_size=ps)
            plain(x, _i32([i] * B), freqs, block_table=pt.table, page_size=ps)
        pools = [getattr(shared, n) for n in ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale") if hasattr(shared, n)]
        pools = [t.view(-1, ps, *t.shape[2:]) for t in pools]
        pairs = [st.fork(0, b, prompt) for b in (1, 2, 3)]
        assert all((p is None) == (prompt % ps == 0) for p in pairs)
        if pairs[0] is not None:
            ops.kv_page_copy(pools[0], pools[1], _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs]), *pools[2:])
        common = st.common_prefix(range(B))
        assert common == prompt // ps * ps and st.num_pages - st.free_pages == (prompt + ps - 1) // ps + 3 * (1 if prompt % ps else 0)
        groups = PrefixGroups(num_groups=2, group_cap=B, max_batch=B, max_prefix=L // 64 * 64, device=DEV, page_table=st)
        groups.set(1, (2, 0, 3, 1), common)
        pos = _i32([prompt] * B)
        for step in range(4):
            for b in range(B):
                st.reserve(b, prompt + step + 1), pt.reserve(b, prompt + step + 1)
            x = _draw(g, B, 1, dtype)
            got = shared.forward_shared(x, pos, freqs, st.table, ps, groups)
            want = plain(x, pos, freqs, block_table=pt.table, page_size=ps)
            assert got.shape == (B, 1, H * DH) and torch.isfinite(got.float()).all() and got.any()
            assert torch.equal(bits(got), bits(want)), step
            pos += 1
        # no groups: the paged forward itself
        x = _draw(g, B, 1, dtype)
        for b in range(B):
            st.reserve(b, prompt + 5), pt.reserve(b, prompt + 5)
        assert torch.equal(bits(shared.forward_shared(x, pos, freqs, st.table, ps, None)), bits(plain(x, pos, freqs, block_table=pt.table, page_size=ps)))
        assert st.num_pages - st.free_pages < pt.num_pages - pt.free_pages
    _forced(64, run)
