"""A mixed packed step on the GPU (awq_attn_varq[_kv8], awq_attn_paged_varq[_kv8]; csrc/awq_varq.hpp "who serves a sequence"): the step
of tests/attn_varq_split_cases.py, dense and through shuffled pages of 64 and 128 keys, T and FP8, at both q tiles, through `ops` and through
the engine binding.  The contract of one call:

    (a) a taken sequence's rows carry the bits of attn_kvcache / attn_kvcache_paged on that sequence alone
    (b) every other row below cu[B] carries the bits of attn_prefill_varq with the same arguments and q tile
    (c) rows >= cu[B] keep what `out` held
    (d) the FP8 call equals the T call on kv8_dequant of the codes
    (e) split_seqlen_q = 0 equals attn_prefill_varq
    (f) two runs give the same bits

and one captured graph (store, then attn_varq) replayed under two steps between which a one-token sequence crosses split_min_keys and another
goes from 1 to 40 new tokens, and the module: forward_packed_split against three rectangular forwards."""
import os
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
from tests import attn_varq_split_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DATA = {}


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def knobs():
    """The split chunk forced to 64 keys (knob attn_splitkv_chunk); returns the setter of the one-pass q tile (knob attn_prefill_rows).  Both
    are restored afterwards."""
    had = os.environ.get("AWQ_TUNING")
    _capi.tune(attn_splitkv_chunk=S.CHUNK)
    yield lambda rows: _capi.tune(attn_prefill_rows=rows)
    _capi.tune(attn_splitkv_chunk=0, attn_prefill_rows=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def _data(dtype, Dh, ps):
    """The step's tensors on the GPU, built once per (dtype, Dh, layout) and never written: q, (k, v) caches or pools, their FP8 codes and
    scales, the T tensors the codes dequantise to, the table (None: dense), cu."""
    key = (dtype, Dh, ps)
    if key not in _DATA:
        st = _DATA.get((dtype, Dh)) or _DATA.setdefault((dtype, Dh), S.Step(dtype, Dh))
        table = None
        k, v = st.k_cache, st.v_cache
        if ps:
            pool = S.Pool(st, ps)
            k, v, table = pool.k_pool, pool.v_pool, pool.table_full.to(DEV)[:, :pool.pps]
            assert table.stride(0) > table.shape[1]
        k, v = k.to(DEV), v.to(DEV)
        # (a row that holds no key has no scale: zeros; nothing of it is read anyway.  The T caches keep their NaN.)
        kq, ks = ops.kv8_quant(k.nan_to_num(0.0))
        vq, vs = ops.kv8_quant(v.nan_to_num(0.0))
        _DATA[key] = SimpleNamespace(st=st, q=st.q.to(DEV), k=k, v=v, kq=kq, vq=vq, ks=ks, vs=vs, kd=ops.kv8_dequant(kq, ks, dtype),
                                     vd=ops.kv8_dequant(vq, vs, dtype), table=table, cu=st.cu_seqlens_q.to(DEV))
    return _DATA[key]


def _sentinel(d):
    return torch.full((d.st.total_q, S.H, d.st.Dh), S.SENTINEL, dtype=d.st.dtype, device=DEV)


def _alone(d, b, lens, before, causal, kv, scales):
    """Sequence b by the rectangular split pair: batch 1, seqlen_q = Sq_b, its own cache row or table row, seqlen_offset = Sq_b under
    lens_before_step, the same bound (and, by the knob, the same chunk)."""
    st = d.st
    one = d.q[st.cu[b]:st.cu[b + 1]][None]
    kw = dict(softmax_scale=None, causal=causal)
    if scales:
        kw.update(k_scale=scales[0] if d.table is not None else scales[0][b:b + 1], v_scale=scales[1] if d.table is not None else scales[1][b:b + 1])
    if d.table is not None:
        return ops.attn_kvcache_paged(one, kv[0], kv[1], d.table[b:b + 1], lens[b:b + 1], S.BOUND, st.offset(b, before), **kw)[0]
    return ops.attn_kvcache(one, kv[0][b:b + 1], kv[1][b:b + 1], lens[b:b + 1], S.BOUND, st.offset(b, before), **kw)[0]


def _check_step(d, fp8, before=True, causal=True, engine=None, tiles=(64, 128), set_tile=None):
    st = d.st
    B, n = len(st.sq), st.cu[-1]
    lens = st.seqlens_k(before).to(DEV)
    kv, scales = ((d.kq, d.vq), (d.ks, d.vs)) if fp8 else ((d.k, d.v), None)
    kw = dict(lens_before_step=before, block_table=d.table, causal=causal)
    if fp8:
        kw.update(k_scale=d.ks, v_scale=d.vs)
    taken = S.routes(before)
    assert taken == S.TAKEN and ops.attn_varq_split_plan(B, S.H, S.HKV, st.Dh, S.SPLIT_SEQLEN_Q, S.BOUND) == (S.BOUND // S.CHUNK, S.CHUNK)
    want_taken = {b: _alone(d, b, lens, before, causal, kv, scales) for b in range(B) if taken[b]}    # (the split pair has no q tile)
    for rows in tiles:
        set_tile(rows)
        assert ops.attn_varq_plan(B, S.H, S.HKV, st.Dh, S.MAX_Q)[0] == rows
        one_pass = ops.attn_prefill_varq(d.q, *kv, d.cu, S.MAX_Q, lens, S.BOUND, out=_sentinel(d), **kw)
        out = ops.attn_varq(d.q, *kv, d.cu, S.MAX_Q, lens, S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS, out=_sentinel(d), **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all(), (rows, "a NaN: a row that holds no key, or a padding row, was read")
        for b in range(B):
            sl = slice(st.cu[b], st.cu[b + 1])
            if taken[b]:      # (a)
                assert out[sl].shape == want_taken[b].shape and out[sl].any()
                assert torch.equal(bits(out[sl]), bits(want_taken[b])), (rows, b, S.STEP[b], "taken: the split pair on the sequence alone")
            else:             # (b)
                assert torch.equal(bits(out[sl]), bits(one_pass[sl])), (rows, b, S.STEP[b], "not taken: the one-pass kernel")
                if not S.active(b):
                    assert not out[sl].any()
        assert (out[n:] == S.SENTINEL).all() and out[n:].shape[0] == S.PAD_ROWS                          # (c)
        again = ops.attn_varq(d.q, *kv, d.cu, S.MAX_Q, lens, S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS, out=_sentinel(d), **kw)
        assert torch.equal(bits(again), bits(out)), (rows, "two runs")                                   # (f)
        none = ops.attn_varq(d.q, *kv, d.cu, S.MAX_Q, lens, S.BOUND, 0, S.SPLIT_MIN_KEYS, out=_sentinel(d), **kw)
        assert torch.equal(bits(none), bits(one_pass)), (rows, "split_seqlen_q = 0")                     # (e)
        if fp8:               # (d)
            t_call = ops.attn_varq(d.q, d.kd, d.vd, d.cu, S.MAX_Q, lens, S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS, out=_sentinel(d),
                                   lens_before_step=before, block_table=d.table, causal=causal)
            assert torch.equal(bits(out), bits(t_call)), (rows, "fp8 against the T call on the dequantised codes")
        if engine is not None:
            eng = engine
            name = "attn" + ("_paged" if d.table is not None else "") + "_varq" + ("_kv8" if fp8 else "")
            where = (*kv, *((d.ks, d.vs) if fp8 else ()), *((d.table,) if d.table is not None else ()))
            e_out = getattr(eng, name)(d.q, *where, d.cu, S.MAX_Q, lens, S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS, before, st.Dh ** -0.5, causal,
                                       _sentinel(d))
            assert torch.equal(bits(e_out), bits(out)), (rows, "the engine binding")
            e_new = getattr(eng, name)(d.q, *where, d.cu, S.MAX_Q, lens, S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS, before, st.Dh ** -0.5, causal)
            assert e_new.shape == out.shape and torch.equal(bits(e_new[:n]), bits(out[:n])), (rows, "the engine binding allocates out")
    return out


LAYOUTS = [0, 64, 128]
LAYOUT_IDS = ["dense", "ps64", "ps128"]


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", S.COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_every_sequence_of_the_step_is_served_by_exactly_one_kernel(dtype, Dh, ps, fp8, knobs):
    _check_step(_data(dtype, Dh, ps), fp8, engine=_engine(), set_tile=knobs)


@pytest.mark.parametrize("ps", [0, 64], ids=["dense", "ps64"])
@pytest.mark.parametrize("dtype,Dh", S.COMBOS[:2], ids=lambda x: str(x).replace("torch.", ""))
def test_the_same_step_under_total_lengths(dtype, Dh, ps, knobs):
    d = _data(dtype, Dh, ps)
    total = _check_step(d, False, before=False, set_tile=knobs, tiles=(64,))
    before = ops.attn_varq(d.q, d.k, d.v, d.cu, S.MAX_Q, d.st.seqlens_k(True).to(DEV), S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS,
                           block_table=d.table, out=_sentinel(d))
    assert torch.equal(bits(total), bits(before))    # either convention names the same lengths: the same routes, the same bits


@pytest.mark.parametrize("ps", [0, 128], ids=["dense", "ps128"])
def test_the_same_step_without_the_causal_mask(ps, knobs):
    d = _data(torch.bfloat16, 128, ps)
    full = _check_step(d, False, causal=False, set_tile=knobs, tiles=(64,))
    causal = ops.attn_varq(d.q, d.k, d.v, d.cu, S.MAX_Q, d.st.seqlens_k(True).to(DEV), S.BOUND, S.SPLIT_SEQLEN_Q, S.SPLIT_MIN_KEYS,
                           block_table=d.table, out=_sentinel(d))
    sl = slice(d.st.cu[3], d.st.cu[4])               # the taken sequence with 8 rows: its first rows see more keys without the mask
    assert not torch.equal(bits(full[sl][:-1]), bits(causal[sl][:-1])) and torch.equal(bits(full[sl][-1]), bits(causal[sl][-1]))


def test_ops_refuse_malformed_calls_on_the_gpu(knobs):
    d = _data(torch.float16, 64, 0)
    lens = d.st.seqlens_k(True).to(DEV)
    for kw, text in ((dict(split_seqlen_q=33), "exceeds 128"), (dict(split_seqlen_q=-1), "must not be negative"), (dict(split_min_keys=0), "at least 1")):
        with pytest.raises(ValueError, match=text):
            ops.attn_varq(d.q, d.k, d.v, d.cu, S.MAX_Q, lens, S.BOUND, **kw)
    with pytest.raises(ValueError, match="packed rows"):
        ops.attn_varq(d.q[None], d.k, d.v, d.cu, S.MAX_Q, lens, S.BOUND)
    eng = _engine()
    for args, text in (((33, 128), "at most 128"), ((-1, 128), "must not be negative"), ((1, 0), "at least 1")):
        with pytest.raises(RuntimeError, match=text):
            eng.attn_varq(d.q, d.k, d.v, d.cu, S.MAX_Q, lens, S.BOUND, *args, True, 0.125, True)


# ------------------------------------------------------------------------------------------------------------------------
# one graph of store + attn_varq at a fixed token budget, replayed under two different steps written in place
# ------------------------------------------------------------------------------------------------------------------------
def _angles(P, Dh):
    inv = 1.0 / (10000.0 ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(P, device=DEV).float(), inv)
    return torch.cat([f, f], -1).contiguous()


def test_one_graph_replays_two_steps_whose_sequences_change_kernels(knobs):
    eng = _engine()
    dtype, Dh, ps, B, T, maxq, L, floor = torch.bfloat16, 128, 64, 4, 144, 128, 256, 64
    W = (S.H + 2 * S.HKV) * Dh
    scale = Dh ** -0.5
    freqs = _angles(L, Dh)
    g = torch.Generator(device=DEV).manual_seed(41)
    pages = B * L // ps
    # sequence 0 brings one token both times and its length crosses the floor upward (63 -> 64 keys); sequence 1 goes from 1 to 40 new tokens
    steps = [dict(sq=(1, 1, 96, 0), pos=(62, 150, 0, 30), table=torch.randperm(pages, generator=torch.Generator().manual_seed(5))),
             dict(sq=(1, 40, 50, 15), pos=(63, 151, 96, 30), table=torch.randperm(pages, generator=torch.Generator().manual_seed(6)))]
    routes = [tuple(S.takes(n, p, True, max_q=maxq, bound=L, split_q=1, floor=floor) for n, p in zip(s["sq"], s["pos"])) for s in steps]
    assert routes == [(False, True, False, False), (True, False, False, False)]
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    table = torch.zeros(B, L // ps, dtype=torch.int32, device=DEV)
    qkv = torch.zeros(T, W, dtype=dtype, device=DEV)
    pools = [(torch.randn(pages, ps, S.HKV, Dh, generator=g, device=DEV)).to(dtype) for _ in range(2)]
    eager = [t.clone() for t in pools]

    def load(s):
        cu.copy_(torch.tensor([0] + list(s["sq"]), dtype=torch.int64).cumsum(0).to(torch.int32))
        pos.copy_(torch.tensor(s["pos"], dtype=torch.int32))
        table.copy_(s["table"].view(B, -1).to(torch.int32))
        qkv.copy_(torch.randn(T, W, generator=g, device=DEV).to(dtype))

    def step(kv):
        xq = eng.rope_kv_store_paged_varq(qkv, freqs, *kv, table, cu, maxq, pos, S.H, S.HKV)
        return eng.attn_paged_varq(xq, *kv, table, cu, maxq, pos, L, 1, floor, True, scale, True)
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
    for s, taken in zip(steps, routes):
        load(s)
        out.fill_(S.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        # eager, per sequence: the store, then the rectangular split pair on a taken sequence alone and the packed one-pass call for the rest
        xq = eng.rope_kv_store_paged_varq(qkv, freqs, *eager, table, cu, maxq, pos, S.H, S.HKV)
        one_pass = eng.attn_prefill_paged_varq(xq, *eager, table, cu, maxq, pos, L, True, scale, True)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(pools, eager))
        lo = 0
        for b, nq in enumerate(s["sq"]):
            sl = slice(lo, lo + nq)
            lo += nq
            if taken[b]:
                want = eng.attn_kvcache_paged(xq[sl][None], *eager, table[b:b + 1], pos[b:b + 1], L, nq, scale, True)[0]
            else:
                want = one_pass[sl]
            assert torch.isfinite(out[sl].float()).all() and torch.equal(bits(out[sl]), bits(want)), (s["sq"], b, taken[b])
        assert lo == sum(s["sq"]) and (out[lo:] == S.SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------------
# the module: 40 / 1 / 96 new tokens in ONE forward_packed_split, against three rectangular forwards
# ------------------------------------------------------------------------------------------------------------------------
HID, H, HKV, DH, L = 512, 8, 2, 64, 256
W = (H + 2 * HKV) * DH
NEW, HIST = (40, 1, 96), (64, 100, 0)
CACHES = ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale")


def _module(kv_dtype=None):
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    # the projections are stand-ins: x already is the qkv tensor and the output is returned as it is
    return QuantLlamaAttentionFused(HID, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=3, kv_layout="natural",
                                    kv_dtype=kv_dtype)


def _draw(g, B, n, dtype):
    mul = torch.cat([torch.full((H * DH,), 1.5), torch.ones(HKV * DH), torch.full((HKV * DH,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * DH), torch.ones(HKV * DH)]).to(DEV)
    return (torch.randn(B, n, W, generator=g, device=DEV) * mul + add).to(dtype)


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_serves_the_decode_of_a_mixed_step_by_the_split_pair(kv_dtype, dtype, paged, knobs):
    knobs(64)
    _capi.tune(attn_splitkv_chunk=0)      # the plan's own chunk, as a server runs it
    assert S.takes(1, 100, True, max_q=96, bound=L, split_q=1, floor=64) and not S.takes(40, 64, True, max_q=96, bound=L, split_q=1, floor=64)
    freqs = _angles(L, DH)
    g = torch.Generator(device=DEV).manual_seed(43)
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
    out = packed.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=1, split_min_keys=64, **kw)
    torch.cuda.synchronize()
    assert out.shape == (1, total + pad, H * DH) and torch.isfinite(out[0, :total].float()).all()
    names = [n for n in CACHES if hasattr(packed, n)]
    after = {n: getattr(packed, n).clone() for n in names}
    # the default call is the existing path: the bits of the packed one-pass attention, which is what split_seqlen_q = 0 launches
    plain = packed.forward_packed(x, pos, freqs, cu, 96, **kw)
    none = packed.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=0, **kw)
    assert torch.equal(bits(plain[0, :total]), bits(none[0, :total]))
    for lo, hi in ((0, 40), (41, 137)):    # the sequences the pair does not take are the existing path's rows
        assert torch.equal(bits(out[0, lo:hi]), bits(plain[0, lo:hi]))
    for n in names:                        # (the three packed forwards stored the same tokens at the same positions)
        assert torch.equal(getattr(packed, n).view(torch.uint8), after[n].view(torch.uint8)), n
    for b, (n, h) in enumerate(zip(NEW, HIST)):
        lo = int(cu[b])
        want = alone(rect, b, x[0, lo:lo + n], h)    # one token: the rectangular forward runs the split pair (attn_kvcache)
        assert torch.equal(bits(out[0, lo:lo + n]), bits(want)), (b, n, h)
        assert torch.equal(bits(plain[0, lo:lo + n]), bits(want)) or n == 1
    assert names and all(getattr(packed, n).view(torch.uint8).any() for n in names)
    for n in names:
        assert torch.equal(getattr(packed, n).view(torch.uint8), getattr(rect, n).view(torch.uint8)), n
