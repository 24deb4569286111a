"""Per-sequence query lengths on the KV-cache path (awq_attn_prefill_kvcache_varq[_kv8], awq_attn_prefill_paged_varq[_kv8],
awq_rope_kv_store_natural_varq[_fp8], awq_rope_kv_store_paged_varq[_fp8]; csrc/awq_varq.hpp): the packed batches of tests/attn_varq_cases.py
bit for bit with every row that must not be written checked, bit-identity of every active sequence to the rectangular kernels on that
sequence alone at both q tiles, the store against the rectangular store per sequence with every other byte of the caches unchanged, random
ragged batches against float64, determinism, one captured graph replayed under two different steps, and the module: three sequences with
40 / 1 / 96 new tokens in ONE packed forward against three rectangular forwards."""
import os
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
from tests import attn_prefill_oracle as O
from tests import attn_varq_cases as V

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


def _sentinel(vb):
    return torch.full((vb.total_q, V.H, vb.q.shape[2]), V.SENTINEL, dtype=vb.dtype, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------
# packed needle batches: bit equality with the CPU targets, rows that must not be written keep the sentinel; dense and paged, T and FP8
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", V.CASES, ids=V.case_id)
def test_packed_batches_bit_exact_on_the_dense_caches(spec, q_tile):
    vb = V.VarqBatch(spec)
    q, kc, vc, cu, lens = (t.to(DEV) for t in (vb.q, vb.k_cache, vb.v_cache, vb.cu_seqlens_q, vb.seqlens_k))
    kw = dict(lens_before_step=vb.before, softmax_scale=vb.scale, causal=vb.causal)
    scale = q.shape[2] ** -0.5 if vb.scale is None else vb.scale
    kq, vq, ks, vs = _quant(kc, vc)
    kd, vd = ops.kv8_dequant(kq, ks, vb.dtype), ops.kv8_dequant(vq, vs, vb.dtype)
    for rows in (64, 128, 0):
        q_tile(rows)
        out = ops.attn_prefill_varq(q, kc, vc, cu, vb.max_q, lens, vb.bound, out=_sentinel(vb), **kw)
        torch.cuda.synchronize()
        assert out.shape == vb.expect.shape and out.is_contiguous()
        _assert_bits(out, vb.expect, ("ops", rows))
        _assert_bits(_engine().attn_prefill_varq(q, kc, vc, cu, vb.max_q, lens, vb.bound, vb.before, scale, vb.causal, _sentinel(vb)), vb.expect,
                     ("engine", rows))
        # FP8: the T form on the dequantised caches, bit for bit
        got = ops.attn_prefill_varq(q, kq, vq, cu, vb.max_q, lens, vb.bound, k_scale=ks, v_scale=vs, out=_sentinel(vb), **kw)
        _assert_bits(got, ops.attn_prefill_varq(q, kd, vd, cu, vb.max_q, lens, vb.bound, out=_sentinel(vb), **kw), ("fp8 against T", rows))
        _assert_bits(_engine().attn_prefill_varq_kv8(q, kq, vq, ks, vs, cu, vb.max_q, lens, vb.bound, vb.before, scale, vb.causal, _sentinel(vb)), got,
                     ("engine fp8", rows))
        if set(vb.sq) == {65}:   # UNIFORM: the rectangular batch call on the same tile, bit for bit
            B, n = len(vb.sq), vb.cu[-1]
            rect = ops.attn_prefill_kvcache(q[:n].view(B, 65, V.H, -1), kc, vc, lens, vb.bound, 65 if vb.before else 0, vb.scale, vb.causal)
            _assert_bits(out[:n], rect.view(n, V.H, -1), ("uniform against the rectangular call", rows))
    if vb.mode != "pair":   # (a pair's mean of two dequantised rows may be a rounding tie: see tests/test_gpu_attention_prefill_kvcache.py)
        vb.k_cache, vb.v_cache = kd.cpu(), vd.cpu()
        _assert_bits(got, V.attend(vb), "fp8 against the CPU restatement")


@pytest.mark.parametrize("spec", V.PAGED_CASES, ids=V.case_id)
def test_packed_batches_bit_exact_through_the_table(spec, q_tile):
    pp = V.PagedVarq(spec)
    vb = pp.batch
    q, cu, lens, kp, vp = (t.to(DEV) for t in (vb.q, vb.cu_seqlens_q, vb.seqlens_k, pp.k_pool, pp.v_pool))
    table = pp.table_full.to(DEV)[:, :pp.pps]  # the row stride stays wider than pages_per_seq
    assert table.stride(0) == pp.pps + V.PAD_COLS
    kw = dict(lens_before_step=vb.before, block_table=table, softmax_scale=vb.scale, causal=vb.causal)
    scale = q.shape[2] ** -0.5 if vb.scale is None else vb.scale
    kq, vq, ks, vs = _quant(kp, vp)
    deq = ops.kv8_dequant(kq, ks, vb.dtype), ops.kv8_dequant(vq, vs, vb.dtype)
    for rows in (64, 128):
        q_tile(rows)
        out = ops.attn_prefill_varq(q, kp, vp, cu, vb.max_q, lens, vb.bound, out=_sentinel(vb), **kw)
        torch.cuda.synchronize()
        _assert_bits(out, vb.expect, ("ops", rows))
        _assert_bits(_engine().attn_prefill_paged_varq(q, kp, vp, table, cu, vb.max_q, lens, vb.bound, vb.before, scale, vb.causal, _sentinel(vb)),
                     vb.expect, ("engine", rows))
        got = ops.attn_prefill_varq(q, kq, vq, cu, vb.max_q, lens, vb.bound, k_scale=ks, v_scale=vs, out=_sentinel(vb), **kw)
        _assert_bits(got, ops.attn_prefill_varq(q, *deq, cu, vb.max_q, lens, vb.bound, out=_sentinel(vb), **kw), ("fp8 against T", rows))
        _assert_bits(_engine().attn_prefill_paged_varq_kv8(q, kq, vq, ks, vs, table, cu, vb.max_q, lens, vb.bound, vb.before, scale, vb.causal,
                                                           _sentinel(vb)), got, ("engine fp8", rows))
    if vb.mode != "pair":
        _assert_bits(got, V.attend(vb, pp=pp, pools=tuple(t.cpu() for t in deq)), "fp8 against the CPU restatement")


def test_flash_attn_varlen_func_serves_a_packed_step_over_the_pool():
    from llm_awq_amd import flash_attn_compat as F

    pp = V.PagedVarq(next(s for s in V.PAGED_CASES if s["name"].startswith("mixed-diag") and s["dtype"] == torch.float16))
    vb = pp.batch
    q, cu, kp, vp = (t.to(DEV) for t in (vb.q, vb.cu_seqlens_q, pp.k_pool, pp.v_pool))
    table = pp.table_full.to(DEV)[:, :pp.pps]
    totals = torch.tensor([0] + vb.total(), dtype=torch.int64).clamp_min(0).cumsum(0).to(torch.int32).to(DEV)   # (the slot at -1 holds 0 keys)
    out = F.flash_attn_varlen_func(q, kp, vp, cu, totals, vb.max_q, vb.bound, causal=True, block_table=table)
    n = vb.cu[-1]
    _assert_bits(out[:n], vb.expect[:n], "shim")


# ------------------------------------------------------------------------------------------------------------------------
# random ragged steps (shared by the tests below, never written to): seven sequences, histories up to 1010, bound 1024, 128-key pages
# ------------------------------------------------------------------------------------------------------------------------
SQS = (200, 1, 37, 0, 130, 64, 17)
HISTS = (700, 333, 0, 57, 100, 960, 1010)   # 960 + 64 fills the bound exactly; 1010 + 17 is beyond it: inactive
MAXQ, BOUND, PS, PADROWS = 200, 1024, 128, 9
COMBOS = [(torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)]
_REF = {}


def _ragged(dtype, Dh, H=8, Hkv=2):
    """q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N: packed q with NaN padding rows, a cache that holds NaN behind every sequence, the same keys in a
    shuffled pool whose unused rows are NaN (table entries behind a live range: the NaN poison page), and the float64 reference of every
    active sequence."""
    key = (dtype, Dh)
    if key not in _REF:
        B = len(SQS)
        cu = [0]
        for n in SQS:
            cu.append(cu[-1] + n)
        lens = [h + n if h + n <= BOUND else None for h, n in zip(HISTS, SQS)]
        g = torch.Generator(device=DEV).manual_seed(Dh + 23)
        q = torch.full((cu[-1] + PADROWS, H, Dh), float("nan"), dtype=dtype, device=DEV)
        q[:cu[-1]] = (1.5 * torch.randn(cu[-1], H, Dh, generator=g, device=DEV)).to(dtype)
        kc = torch.full((B, BOUND + 9, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
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
            if n is None or SQS[b] == 0:
                refs.append(None)
                if n is None:
                    continue
            kc[b, :n] = torch.randn(n, Hkv, Dh, generator=g, device=DEV).to(dtype)
            vc[b, :n] = (1 + 0.5 * torch.randn(n, Hkv, Dh, generator=g, device=DEV)).to(dtype)
            for i in range(need[b]):
                page = order.pop()
                full[b, i] = page
                rows = min(PS, n - i * PS)
                kp[page, :rows], vp[page, :rows] = kc[b, i * PS:i * PS + rows], vc[b, i * PS:i * PS + rows]
            if SQS[b]:
                refs.append(O.attention(q[None, cu[b]:cu[b + 1]], kc[b:b + 1, :n], vc[b:b + 1, :n], None, True, stats=True))
        hist = torch.tensor(HISTS, dtype=torch.int32, device=DEV)
        cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
        _REF[key] = (q, kc, vc, kp, vp, full.to(DEV)[:, :pps], hist, cu_t, cu, lens, refs)
    return _REF[key]


@pytest.mark.parametrize("dtype,Dh", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_random_ragged_steps_against_float64(dtype, Dh):
    q, kc, vc, kp, vp, table, hist, cu_t, cu, lens, refs = _ragged(dtype, Dh)
    dense = ops.attn_prefill_varq(q, kc, vc, cu_t, MAXQ, hist, BOUND)
    paged = ops.attn_prefill_varq(q, kp, vp, cu_t, MAXQ, hist, BOUND, block_table=table)
    n = cu[-1]
    assert torch.isfinite(dense[:n].float()).all() and torch.equal(bits(dense[:n]), bits(paged[:n]))
    for b, tot in enumerate(lens):
        rows = dense[cu[b]:cu[b + 1]]
        if tot is None:
            assert rows.shape[0] == SQS[b] and not rows.view(torch.int16).any()
            continue
        if refs[b] is None:
            continue
        ref, A, qk = refs[b]
        lim = O.bound(ref, A, qk, dtype, tot, Dh, Dh ** -0.5)
        err = (rows[None].double() - ref).abs()
        print(f"{dtype} Dh {Dh} Sq {SQS[b]} Sk {tot}: max err / bound = {float((err / lim).max()):.3f}")
        assert not (err > lim).any(), (b, tot, float((err / lim).max()))


@pytest.mark.parametrize("dtype,Dh", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_every_active_sequence_is_bit_identical_to_the_rectangular_kernel_on_it_alone(dtype, Dh, q_tile):
    """The reference is the parent's device-length one-pass entry on one sequence: batch 1, seqlen_q = Sq_b, its own length, its own table
    row.  Forcing the q tile keeps both calls on one tile."""
    q, kc, vc, kp, vp, table, hist, cu_t, cu, lens, _ = _ragged(dtype, Dh)
    kq, vq, ks, vs = _quant(kp, vp)
    ckq, cvq, cks, cvs = _quant(kc, vc)
    for rows in (64, 128):
        q_tile(rows)
        assert ops.attn_varq_plan(len(SQS), 8, 2, Dh, MAXQ)[0] == rows
        dense = ops.attn_prefill_varq(q, kc, vc, cu_t, MAXQ, hist, BOUND)
        paged = ops.attn_prefill_varq(q, kp, vp, cu_t, MAXQ, hist, BOUND, block_table=table)
        dense8 = ops.attn_prefill_varq(q, ckq, cvq, cu_t, MAXQ, hist, BOUND, k_scale=cks, v_scale=cvs)
        paged8 = ops.attn_prefill_varq(q, kq, vq, cu_t, MAXQ, hist, BOUND, block_table=table, k_scale=ks, v_scale=vs)
        total = ops.attn_prefill_varq(q, kc, vc, cu_t, MAXQ, hist + torch.tensor(SQS, dtype=torch.int32, device=DEV), BOUND, lens_before_step=False)
        for b, n in enumerate(lens):
            if n is None or SQS[b] == 0:
                continue
            sl = slice(cu[b], cu[b + 1])
            one = q[sl][None]
            assert ops.attn_prefill_plan(1, 8, 2, Dh, SQS[b], BOUND)[0] == rows
            want = ops.attn_prefill_kvcache(one, kc[b:b + 1], vc[b:b + 1], hist[b:b + 1], BOUND, SQS[b])[0]
            assert torch.equal(bits(dense[sl]), bits(want)), (rows, b, "dense")
            assert torch.equal(bits(total[sl]), bits(want)), (rows, b, "dense, total lengths")
            assert torch.equal(bits(paged[sl]), bits(ops.attn_prefill_paged(one, kp, vp, table[b:b + 1], hist[b:b + 1], BOUND, SQS[b])[0])), (rows, b, "paged")
            want8 = ops.attn_prefill_kvcache(one, ckq[b:b + 1], cvq[b:b + 1], hist[b:b + 1], BOUND, SQS[b], k_scale=cks[b:b + 1], v_scale=cvs[b:b + 1])[0]
            assert torch.equal(bits(dense8[sl]), bits(want8)), (rows, b, "dense fp8")
            want8 = ops.attn_prefill_paged(one, kq, vq, table[b:b + 1], hist[b:b + 1], BOUND, SQS[b], k_scale=ks, v_scale=vs)[0]
            assert torch.equal(bits(paged8[sl]), bits(want8)), (rows, b, "paged fp8")


def test_same_call_twice_gives_the_same_bits_and_a_loose_bound_changes_nothing():
    dtype, Dh = torch.bfloat16, 128
    q, kc, vc, kp, vp, table, hist, cu_t, cu, lens, _ = _ragged(dtype, Dh)
    n = cu[-1]
    for fn in (lambda m: ops.attn_prefill_varq(q, kc, vc, cu_t, m, hist, BOUND), lambda m: ops.attn_prefill_varq(q, kp, vp, cu_t, m, hist, BOUND, block_table=table)):
        a, b, loose = fn(MAXQ), fn(MAXQ), fn(1000)
        assert torch.equal(bits(a[:n]), bits(b[:n])) and a[:n].any()
        assert ops.attn_varq_plan(len(SQS), 8, 2, Dh, MAXQ)[0] == ops.attn_varq_plan(len(SQS), 8, 2, Dh, 1000)[0]
        assert torch.equal(bits(a[:n]), bits(loose[:n]))     # whole ranks of empty blocks, the same rows


def test_ops_refuse_malformed_packed_tensors():
    q, kc, vc, kp, vp, table, hist, cu_t, cu, lens, _ = _ragged(torch.float16, 64)
    with pytest.raises(ValueError, match="packed rows"):
        ops.attn_prefill_varq(q[None], kc, vc, cu_t, MAXQ, hist, BOUND)
    with pytest.raises(ValueError, match=r"\[B \+ 1\]"):
        ops.attn_prefill_varq(q, kc, vc, cu_t.long(), MAXQ, hist, BOUND)
    with pytest.raises(ValueError, match=r"int32 \[B\]"):
        ops.attn_prefill_varq(q, kc, vc, cu_t, MAXQ, hist[:-1], BOUND)
    with pytest.raises(ValueError, match="total_q, H, Dh"):
        ops.attn_prefill_varq(q, kc, vc, cu_t, MAXQ, hist, BOUND, out=torch.empty(3, 8, 64, dtype=q.dtype, device=DEV))
    with pytest.raises(RuntimeError, match="cu_seqlens_q"):
        _engine().attn_prefill_varq(q, kc, vc, cu_t.long(), MAXQ, hist, BOUND, True, 0.125, True)


# ------------------------------------------------------------------------------------------------------------------------
# the store: per sequence the rectangular store's bits, every other byte of the caches unchanged, padding rows keep the sentinel
# ------------------------------------------------------------------------------------------------------------------------
STORE_CASES = [s for s in V.CASES if s["before"] and s["mode"] in ("diag", "scatter")]


def _angles(P, Dh):
    inv = 1.0 / (10000.0 ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(P, device=DEV).float(), inv)
    return torch.cat([f, f], -1).contiguous()


def _fill(shape, dtype, seed):
    """A cache full of bytes nobody would store: finite T values, or codes / scales of a fixed pattern."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if dtype == torch.float32:
        return torch.rand(shape, generator=g, device=DEV) + 7.0
    if dtype == torch.uint8:
        return torch.randint(0, 120, shape, generator=g, device=DEV, dtype=torch.uint8)
    return (torch.rand(shape, generator=g, device=DEV) + 9.0).to(dtype)


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("spec", STORE_CASES, ids=V.case_id)
def test_store_is_the_rectangular_store_per_sequence_and_touches_nothing_else(spec, paged, fp8):
    pp = V.PagedVarq(dict(spec, page_size=64))
    vb = pp.batch
    Dh, dt, B, T = vb.q.shape[2], vb.dtype, len(vb.sq), vb.total_q
    W = (V.H + 2 * V.HKV) * Dh
    freqs = _angles(V.BOUND, Dh)   # BOUND table rows: the sequence one key beyond the bound is inactive on the dense caches too
    g = torch.Generator(device=DEV).manual_seed(T + Dh)
    qkv = torch.full((T, W), float("nan"), dtype=dt, device=DEV)
    qkv[:vb.cu[-1]] = torch.randn(vb.cu[-1], W, generator=g, device=DEV).to(dt)
    cu, pos = vb.cu_seqlens_q.to(DEV), vb.seqlens_k.to(DEV)
    table = pp.table_full.to(DEV)[:, :pp.pps]
    shape = (pp.num_pages, pp.ps, V.HKV, Dh) if paged else (B, vb.lmax, V.HKV, Dh)
    cdt = torch.uint8 if fp8 else dt
    init = [_fill(shape, cdt, 1), _fill(shape, cdt, 2)] + ([_fill(shape[:3], torch.float32, 3), _fill(shape[:3], torch.float32, 4)] if fp8 else [])
    got, ref = [t.clone() for t in init], [t.clone() for t in init]
    kw = dict(block_table=table) if paged else {}

    def scales(ts):
        return dict(k_scale=ts[2], v_scale=ts[3]) if fp8 else {}
    q_out = ops.rope_kv_store_varq(qkv, freqs, got[0], got[1], cu, vb.max_q, pos, V.H, V.HKV, q_out=_sentinel(vb), **kw, **scales(got))
    torch.cuda.synchronize()
    want_q = _sentinel(vb)
    where = V.store_expect(vb)
    for b, nq in enumerate(vb.sq):
        if nq == 0:
            continue
        sl = slice(vb.cu[b], vb.cu[b + 1])
        if where[vb.cu[b]] is None:        # inactive: zero q rows, nothing stored
            want_q[sl] = 0
            continue
        one = qkv[sl][None]
        if paged:
            want_q[sl] = ops.rope_kv_store_paged(one, freqs, ref[0], ref[1], table[b:b + 1], pos[b:b + 1], V.H, V.HKV, **scales(ref))[0]
        else:
            sc = dict(k_scale=ref[2][b:b + 1], v_scale=ref[3][b:b + 1]) if fp8 else {}
            want_q[sl] = ops.rope_kv_store_natural_pos(one, freqs, ref[0][b:b + 1], ref[1][b:b + 1], pos[b:b + 1], V.H, V.HKV, **sc)[0]
    torch.cuda.synchronize()
    _assert_bits(q_out, want_q, "q_out: the rectangular rows, zeros for inactive sequences, the sentinel in the padding")
    written = torch.zeros(shape[:2], dtype=torch.bool, device=DEV)
    for e in where:
        if e is not None:
            b, p = e
            written[(int(table[b, p // pp.ps]), p % pp.ps) if paged else (b, p)] = True
    assert int(written.sum()) == sum(e is not None for e in where) > 0
    for name, a, r, i in zip(("k", "v", "k_scale", "v_scale"), got, ref, init):
        assert torch.equal(a.view(torch.uint8), r.view(torch.uint8)), name                       # the rectangular store's bytes
        assert torch.equal(a[~written].view(torch.uint8), i[~written].view(torch.uint8)), name   # every other row as it was
        assert not torch.equal(a[written].view(torch.uint8), i[written].view(torch.uint8)), name
    eng = _engine()
    again = [t.clone() for t in init]
    if paged:
        fn = eng.rope_kv_store_paged_varq_fp8 if fp8 else eng.rope_kv_store_paged_varq
        eq = fn(qkv, freqs, *again, table, cu, vb.max_q, pos, V.H, V.HKV, _sentinel(vb))
    else:
        fn = eng.rope_kv_store_natural_varq_fp8 if fp8 else eng.rope_kv_store_natural_varq
        eq = fn(qkv, freqs, *again, cu, vb.max_q, pos, V.H, V.HKV, _sentinel(vb))
    _assert_bits(eq, want_q, "engine q_out")
    assert all(torch.equal(a.view(torch.uint8), r.view(torch.uint8)) for a, r in zip(again, got))


# ------------------------------------------------------------------------------------------------------------------------
# one graph of store + attention at a fixed token budget, replayed under two different steps written in place
# ------------------------------------------------------------------------------------------------------------------------
def test_one_graph_replays_two_different_packed_steps():
    eng = _engine()
    dtype, Dh, ps, B, T, maxq, L = torch.bfloat16, 128, 64, 4, 144, 128, 256
    W = (V.H + 2 * V.HKV) * Dh
    freqs = _angles(L, Dh)
    g = torch.Generator(device=DEV).manual_seed(29)
    pages = B * L // ps
    steps = [dict(sq=(40, 1, 96, 0), pos=(10, 77, 0, 30), table=torch.randperm(pages, generator=torch.Generator().manual_seed(1))),
             dict(sq=(1, 1, 120, 15), pos=(50, 78, 96, 30), table=torch.randperm(pages, generator=torch.Generator().manual_seed(2)))]
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    table = torch.zeros(B, L // ps, dtype=torch.int32, device=DEV)
    qkv = torch.zeros(T, W, dtype=dtype, device=DEV)
    pools = [(torch.randn(pages, ps, V.HKV, Dh, generator=g, device=DEV)).to(dtype) for _ in range(2)]
    eager = [t.clone() for t in pools]

    def load(s):
        cu.copy_(torch.tensor([0] + list(s["sq"]), dtype=torch.int64).cumsum(0).to(torch.int32))
        pos.copy_(torch.tensor(s["pos"], dtype=torch.int32))
        table.copy_(s["table"].view(B, -1).to(torch.int32))
        qkv.copy_(torch.randn(T, W, generator=g, device=DEV).to(dtype))

    def step(kv):
        xq = eng.rope_kv_store_paged_varq(qkv, freqs, *kv, table, cu, maxq, pos, V.H, V.HKV)
        return eng.attn_prefill_paged_varq(xq, *kv, table, cu, maxq, pos, L, True, Dh ** -0.5, True)
    load(steps[0])
    scratch = [t.clone() for t in pools]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, on pools of its own
        step(scratch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(pools)
    for pools_t, e in zip(pools, eager):   # (the capture itself launched nothing)
        assert torch.equal(bits(pools_t), bits(e))
    seen = []
    for s in steps:
        load(s)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = step(eager)
        n = sum(s["sq"])
        assert torch.isfinite(out[:n].float()).all() and torch.equal(bits(out[:n]), bits(want[:n])), s["sq"]
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(pools, eager))
        seen.append(out[:n].clone())
    assert seen[0].shape != seen[1].shape or not torch.equal(bits(seen[0]), bits(seen[1]))


# ------------------------------------------------------------------------------------------------------------------------
# the module: 40 / 1 / 96 new tokens over different histories in ONE packed forward, against three rectangular forwards
# ------------------------------------------------------------------------------------------------------------------------
HID, H, HKV, DH, L = 512, 8, 2, 64, 256
W = (H + 2 * HKV) * DH
NEW, HIST = (40, 1, 96), (64, 100, 0)
CACHES = ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale")


def _module(kv_dtype=None):
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    # the projections are stand-ins (tests/test_gpu_chunk_prefill.py): x already is the qkv tensor and the output is returned as it is
    return QuantLlamaAttentionFused(HID, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=3, kv_layout="natural",
                                    kv_dtype=kv_dtype)


def _draw(g, B, S, dtype):
    mul = torch.cat([torch.full((H * DH,), 1.5), torch.ones(HKV * DH), torch.full((HKV * DH,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * DH), torch.ones(HKV * DH)]).to(DEV)
    return (torch.randn(B, S, W, generator=g, device=DEV) * mul + add).to(dtype)


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("rows", [64, 128])
def test_module_takes_three_sequences_in_one_packed_forward(kv_dtype, dtype, paged, rows, q_tile):
    q_tile(rows)
    freqs = _angles(L, DH)
    g = torch.Generator(device=DEV).manual_seed(31)
    packed, rect = _module(kv_dtype), _module(kv_dtype)
    kw = {}
    if paged:
        ps = 64
        kw = dict(block_table=torch.randperm(3 * L // ps, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(3, -1).to(DEV), page_size=ps)

    def alone(m, b, x, p):
        """Sequence b's rectangular forward: the other slots sit the call out (start_pos -1)."""
        xs = torch.zeros(3, x.shape[0], W, dtype=dtype, device=DEV)
        xs[b] = x
        at = torch.full((3,), -1, dtype=torch.int32, device=DEV)
        at[b] = p
        return m(xs, at, freqs, **kw)[b]
    for b, h in enumerate(HIST):   # the histories, by the same rectangular calls on both modules
        if h:
            x = _draw(g, 1, h, dtype)[0]
            alone(packed, b, x, 0), alone(rect, b, x, 0)
    total, pad = sum(NEW), 7
    x = torch.full((1, total + pad, W), float("nan"), dtype=dtype, device=DEV)
    x[0, :total] = _draw(g, 1, total, dtype)[0]
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32, device=DEV)
    pos = torch.tensor(HIST, dtype=torch.int32, device=DEV)
    out = packed.forward_packed(x, pos, freqs, cu, 96, **kw)
    torch.cuda.synchronize()
    assert out.shape == (1, total + pad, H * DH) and torch.isfinite(out[0, :total].float()).all()
    for b, (n, h) in enumerate(zip(NEW, HIST)):
        lo = int(cu[b])
        want = alone(rect, b, x[0, lo:lo + n], h)
        same = torch.equal(bits(out[0, lo:lo + n]), bits(want))
        print(f"sequence {b}: {n} new tokens over {h}: output bits equal = {same}")
        assert same, (b, n, h)
    names = [n for n in CACHES if hasattr(packed, n)]
    assert names and all(getattr(packed, n).view(torch.uint8).any() for n in names)
    for n in names:
        assert torch.equal(getattr(packed, n).view(torch.uint8), getattr(rect, n).view(torch.uint8)), n
    # the rows of the sequences' last tokens, as the LM head takes them: a device gather
    last = out[0, (cu[1:] - 1).long()]
    assert last.shape == (3, H * DH) and torch.equal(bits(last[2]), bits(out[0, 136]))
