"""Sliding-window attention on packed steps on the GPU (awq_attn_varq_window[_kv8], awq_attn_paged_varq_window[_kv8]; csrc/awq_window.hpp):
the step of tests/attn_window_cases.py under every window of LEFTS, dense and through shuffled pages of 64 and 128 keys, T and FP8.

    1. every row within attn_prefill_oracle.bound of the float64 oracle, under the rule's routes (split_min_keys 128) and with every short
       sequence forced onto the split pair (split_min_keys 1); inactive slots zeros, padding rows untouched
    2. a window that hides nothing returns the bits of attn_varq without a window, on both routes
    3. a one-token sequence whose window starts at a multiple of the page returns the bits of the unwindowed call on the window's keys moved
       to position 0, on both routes
    4. every sequence's rows are those of the windowed call on that sequence alone under the route written down by hand
    5. nothing below a sequence's first tile is read: NaN keys, NaN scales and a poison page there change no bit; large finite values
       between the tile start and the first window start stay inside the bound
    6. one captured graph replays two steps with different lengths and routes, and again after release_before rewrote the table in place"""
import os
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.paged_kv import PageTable
from tests import attn_prefill_oracle as P
from tests import attn_window_cases as W
from tests import attn_window_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DATA, _REF = {}, {}
LAYOUTS = [0, 64, 128]
LAYOUT_IDS = ["dense", "ps64", "ps128"]
IDS = lambda x: str(x).replace("torch.", "")


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def knobs():
    """The split chunk forced to 64 keys and the one-pass q tile to 128 rows (four waves: the 130-row chunk's rows start in three tiles);
    returns the setter of the q tile.  Both are restored afterwards."""
    had = os.environ.get("AWQ_TUNING")
    _capi.tune(attn_splitkv_chunk=W.CHUNK, attn_prefill_rows=128)
    yield lambda rows: _capi.tune(attn_prefill_rows=rows)
    _capi.tune(attn_splitkv_chunk=0, attn_prefill_rows=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def _layout(st, k_cache, v_cache, ps):
    """(k, v, table) on the GPU: the caches, or S.Pool's shuffled pages of them."""
    if not ps:
        return k_cache.to(DEV), v_cache.to(DEV), None
    view = SimpleNamespace(held=st.held, Dh=st.Dh, dtype=st.dtype, k_cache=k_cache, v_cache=v_cache)
    pool = W.S.Pool(view, ps)
    table = pool.table_full.to(DEV)[:, :pool.pps]
    assert table.stride(0) > table.shape[1]
    return pool.k_pool.to(DEV), pool.v_pool.to(DEV), table


def _pack(st, k, v, table, dtype):
    kq, ks = ops.kv8_quant(k.nan_to_num(0.0))
    vq, vs = ops.kv8_quant(v.nan_to_num(0.0))
    return SimpleNamespace(st=st, q=st.q.to(DEV), k=k, v=v, kq=kq, vq=vq, ks=ks, vs=vs, table=table, cu=st.cu_seqlens_q.to(DEV),
                           lens=st.seqlens_k(True).to(DEV))


def _data(dtype, Dh, ps):
    """The step's tensors on the GPU, built once per (dtype, Dh, layout) and never written."""
    key = (dtype, Dh, ps)
    if key not in _DATA:
        st = _DATA.get((dtype, Dh)) or _DATA.setdefault((dtype, Dh), W.Step(dtype, Dh))
        _DATA[key] = _pack(st, *_layout(st, st.k_cache, st.v_cache, ps), dtype)
    return _DATA[key]


def _reference(dtype, Dh, fp8, left):
    """Per active sequence (ref, bound), float64 on the CPU, once per (dtype, Dh, cache format, left): the oracle on the T caches, or on what
    the FP8 codes of the dense caches dequantise to (one scale per (key, KV head): the pages hold the same codes)."""
    key = (dtype, Dh, fp8, left)
    if key not in _REF:
        d = _data(dtype, Dh, 0)
        st = d.st
        k, v = (ops.kv8_dequant(d.kq, d.ks, dtype).cpu(), ops.kv8_dequant(d.vq, d.vs, dtype).cpu()) if fp8 else (st.k_cache, st.v_cache)
        out = {}
        for b, (n, h) in enumerate(W.STEP):
            if W.active(b) and n:
                ref, A, qk = O.attention(*st.seq(b, k, v), left, stats=True)
                out[b] = (ref[0], P.bound(ref, A, qk, dtype, h + n, Dh, Dh ** -0.5)[0])
        _REF[key] = out
    return _REF[key]


def _sentinel(d):
    return torch.full((d.st.total_q, W.H, d.st.Dh), W.SENTINEL, dtype=d.st.dtype, device=DEV)


def _run(d, fp8, left, floor=W.SPLIT_MIN_KEYS, split_q=W.SPLIT_SEQLEN_Q, out=None):
    kv = (d.kq, d.vq) if fp8 else (d.k, d.v)
    kw = dict(k_scale=d.ks, v_scale=d.vs) if fp8 else {}
    kw.update(block_table=d.table, out=_sentinel(d) if out is None else out)
    if left is None:   # the call without a window
        return ops.attn_varq(d.q, *kv, d.cu, W.MAX_Q, d.lens, W.BOUND, split_q, floor, **kw)
    return ops.attn_varq_window(d.q, *kv, d.cu, W.MAX_Q, d.lens, W.BOUND, left, split_q, floor, **kw)


def _check_against_oracle(d, fp8, out, left, what):
    st = d.st
    n_rows = st.cu[-1]
    refs = _reference(st.dtype, st.Dh, fp8, left)
    assert torch.isfinite(out.float()).all(), (what, "a NaN: a row that holds no key, or a padding row, was read")
    o = out.double().cpu()
    for b, (n, h) in enumerate(W.STEP):
        sl = slice(st.cu[b], st.cu[b + 1])
        if b in refs:
            ref, bound = refs[b]
            err = (o[sl] - ref).abs()
            worst = float((err / bound).max())
            print(f"{what} left {left} seq {b} {W.STEP[b]}: worst |err| / bound = {worst:.3f}")
            assert bool((err <= bound).all()), (what, left, b, W.STEP[b], worst)
        else:
            assert not out[sl].any(), (what, left, b, "an inactive slot's rows are zeros")
    assert (out[n_rows:] == W.SENTINEL).all() and out[n_rows:].shape[0] == W.PAD_ROWS


# ------------------------------------------------------------------------------------------------------------------------
# 1. the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", W.COMBOS, ids=IDS)
def test_every_row_is_within_the_bound_of_the_oracle(dtype, Dh, ps, fp8, knobs):
    d = _data(dtype, Dh, ps)
    assert ops.attn_varq_plan(len(W.STEP), W.H, W.HKV, Dh, W.MAX_Q)[0] == 128
    for left in W.LEFTS:
        assert W.routes(left) == W.TAKEN[left]
        _check_against_oracle(d, fp8, _run(d, fp8, left), left, "rule")
        _check_against_oracle(d, fp8, _run(d, fp8, left, floor=1), left, "forced")     # every short sequence on the split pair
    knobs(64)                                                                          # the 64-row q tile: two waves, other tile edges
    for left in (63, 100):
        _check_against_oracle(d, fp8, _run(d, fp8, left), left, "rows64")


# ------------------------------------------------------------------------------------------------------------------------
# 2. a window that hides nothing
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", W.COMBOS[:2], ids=IDS)
def test_a_window_that_covers_the_bound_returns_the_bits_without_a_window(dtype, Dh, ps, fp8, knobs):
    d = _data(dtype, Dh, ps)
    for floor, split_q in ((W.SPLIT_MIN_KEYS, W.SPLIT_SEQLEN_Q), (1, W.SPLIT_SEQLEN_Q), (W.SPLIT_MIN_KEYS, 0)):
        plain = _run(d, fp8, None, floor, split_q)
        assert plain[:d.st.cu[-1]].any()
        for left in (W.BOUND - 1, W.BOUND, 10 ** 6, 2 ** 31 - 1):
            assert torch.equal(bits(_run(d, fp8, left, floor, split_q)), bits(plain)), (floor, split_q, left)
    assert not torch.equal(bits(_run(d, fp8, W.BOUND - 2)), bits(_run(d, fp8, None)))      # one key less: sequence 7 fills the bound


# ------------------------------------------------------------------------------------------------------------------------
# 3. the window's keys moved to position 0
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", W.COMBOS[:2], ids=IDS)
def test_a_decode_equals_the_unwindowed_call_on_the_windows_keys_moved_to_key_0(dtype, Dh, ps, fp8, knobs):
    d = _data(dtype, Dh, ps)
    st = d.st
    b, left = 0, 128                       # Sk_b = 257: the window is keys 128 .. 256, a multiple of every page size and of the tile
    n, h = W.STEP[b]
    start = h - left
    assert n == 1 and start == 128 and start % 128 == 0
    q = d.q[st.cu[b]:st.cu[b + 1]]
    cu = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    kv = (d.kq, d.vq, d.ks, d.vs) if fp8 else (d.k, d.v)
    if ps:
        here, moved, table, table0 = kv, kv, d.table[b:b + 1], d.table[b:b + 1, start // ps:]
    else:
        here, moved, table, table0 = tuple(t[b:b + 1] for t in kv), tuple(t[b:b + 1, start:] for t in kv), None, None
    sc = lambda t: dict(k_scale=t[2], v_scale=t[3]) if fp8 else {}
    for floor, split_q in ((1, W.SPLIT_SEQLEN_Q), (W.SPLIT_MIN_KEYS, 0)):          # once on each route
        lens = torch.tensor([h], dtype=torch.int32, device=DEV)
        win = ops.attn_varq_window(q, *here[:2], cu, 1, lens, W.BOUND, left, split_q, floor, block_table=table, **sc(here))
        lens0 = torch.tensor([h - start], dtype=torch.int32, device=DEV)
        bound0 = W.BOUND - start
        ref = ops.attn_varq(q, *moved[:2], cu, 1, lens0, bound0, split_q, floor, block_table=table0, **sc(moved))
        assert win.any() and torch.equal(bits(win), bits(ref)), (floor, split_q)
        full = ops.attn_varq(q, *here[:2], cu, 1, lens, W.BOUND, split_q, floor, block_table=table, **sc(here))
        assert not torch.equal(bits(win), bits(full))


# ------------------------------------------------------------------------------------------------------------------------
# 4. the routes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", W.COMBOS[:2], ids=IDS)
def test_every_sequence_is_served_by_the_route_written_down_by_hand(dtype, Dh, ps, fp8, knobs):
    d = _data(dtype, Dh, ps)
    st = d.st
    kv = (d.kq, d.vq, d.ks, d.vs) if fp8 else (d.k, d.v)
    for left in (1, 100, 191):
        out = _run(d, fp8, left)
        for b, (n, h) in enumerate(W.STEP):
            if not n:
                continue
            sl = slice(st.cu[b], st.cu[b + 1])
            one = kv if ps else tuple(t[b:b + 1] for t in kv)
            cu = torch.tensor([0, n], dtype=torch.int32, device=DEV)
            taken = W.TAKEN[left][b]
            # alone, on the route written down: the split pair whatever the keys (floor 1), or the one-pass kernel alone (split_seqlen_q 0)
            alone = ops.attn_varq_window(d.q[sl], *one[:2], cu, W.MAX_Q, d.lens[b:b + 1], W.BOUND, left, W.SPLIT_SEQLEN_Q if taken else 0, 1,
                                  block_table=d.table[b:b + 1] if ps else None,
                                  **(dict(k_scale=one[2], v_scale=one[3]) if fp8 else {}))
            assert torch.equal(bits(out[sl]), bits(alone)), (left, b, W.STEP[b], taken)
    eng = _engine()                       # the engine binding gives the bits of ops
    name = "attn" + ("_paged" if ps else "") + "_varq_window" + ("_kv8" if fp8 else "")
    where = (*kv, *((d.table,) if ps else ()))
    e_out = getattr(eng, name)(d.q, *where, d.cu, W.MAX_Q, d.lens, W.BOUND, W.SPLIT_SEQLEN_Q, W.SPLIT_MIN_KEYS, 191, True, Dh ** -0.5, True, _sentinel(d))
    assert torch.equal(bits(e_out), bits(out))


# ------------------------------------------------------------------------------------------------------------------------
# 5. dead keys
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("ps", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype,Dh", W.COMBOS[:2], ids=IDS)
def test_nothing_below_a_sequences_first_tile_is_read(dtype, Dh, ps, fp8, knobs):
    clean = _data(dtype, Dh, ps)
    st = clean.st
    nan = float("nan")
    for left in (0, 63, 100, 191):
        k, v = st.k_cache.clone(), st.v_cache.clone()
        big_k, big_v = st.k_cache.clone(), st.v_cache.clone()
        dead = 0
        for b, (n, h) in enumerate(W.STEP):
            if not (W.active(b) and n):
                continue
            a = W.anchor(b, left)
            k[b, :a], v[b, :a] = nan, nan
            dead += a
            first = max(0, h - left)      # the window start of the sequence's first row: keys a .. first - 1 are read and masked
            big_k[b, a:first], big_v[b, a:first] = 300.0, -300.0
        assert dead > 0
        d = _pack(st, *_layout(st, k, v, ps), dtype)
        if fp8:                            # NaN codes (e4m3fn 0x7F) and NaN scales wherever the T cache holds NaN
            hole = torch.isnan(d.k.float()).all(-1)
            for codes, scales in ((d.kq, d.ks), (d.vq, d.vs)):
                codes.view(torch.uint8)[hole] = 0x7F
                scales[hole] = nan
        if ps:                             # every table entry below the first tile names the all-NaN poison page
            pool = W.S.Pool(SimpleNamespace(held=st.held, Dh=st.Dh, dtype=st.dtype, k_cache=k, v_cache=v), ps)
            table = d.table.clone()
            for b, (n, h) in enumerate(W.STEP):
                if W.active(b) and n:
                    table[b, :W.anchor(b, left) // ps] = pool.poison
            assert torch.isnan(d.k[pool.poison].float()).all()
            d.table = table
        for floor in (W.SPLIT_MIN_KEYS, 1):
            want = _run(clean, fp8, left, floor)
            got = _run(d, fp8, left, floor)
            assert torch.isfinite(got.float()).all() and torch.equal(bits(got), bits(want)), (left, floor)
        big = _pack(st, *_layout(st, big_k, big_v, ps), dtype)
        for floor in (W.SPLIT_MIN_KEYS, 1):
            # a masked key's weight is exactly 0 and one FP8 scale serves one key: the clean reference stands
            _check_against_oracle(big, fp8, _run(big, fp8, left, floor), left, "big")


# ------------------------------------------------------------------------------------------------------------------------
# 6. one graph: two steps, then the table rewritten in place by release_before
# ------------------------------------------------------------------------------------------------------------------------
def _angles(Pn, Dh):
    inv = 1.0 / (10000.0 ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(Pn, device=DEV).float(), inv)
    return torch.cat([f, f], -1).contiguous()


def test_one_graph_replays_two_steps_and_follows_release_before(knobs):
    eng = _engine()
    dtype, Dh, ps, B, T, maxq, L, floor, left = torch.bfloat16, 128, 64, 3, 80, 64, 512, 64, 100
    Wd = (W.H + 2 * W.HKV) * Dh
    scale = Dh ** -0.5
    freqs = _angles(L, Dh)
    g = torch.Generator(device=DEV).manual_seed(47)
    pt = PageTable(num_pages=B * L // ps, page_size=ps, max_batch=B, pages_per_seq=L // ps, device=DEV)
    # sequence 0 decodes over 300 keys (keys_b = 101 >= 64: the split pair), then over 40 (keys_b = 41: one-pass); sequence 1 brings a
    # 40-token chunk, then decodes over 301 keys; sequence 2 idles, then brings 30 tokens
    steps = [dict(sq=(1, 40, 0), pos=(300, 0, 50)), dict(sq=(1, 1, 30), pos=(40, 301, 50))]
    routes = [tuple(O.takes(n, p, True, left, maxq, L, 1, floor) for n, p in zip(s["sq"], s["pos"])) for s in steps]
    assert routes == [(True, False, False), (False, True, False)]
    for b, need in enumerate((400, 400, 200)):
        pt.reserve(b, need)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    qkv = torch.zeros(T, Wd, dtype=dtype, device=DEV)
    pools = [torch.randn(pt.num_pages, ps, W.HKV, Dh, generator=g, device=DEV).to(dtype) for _ in range(2)]

    def load(s):
        cu.copy_(torch.tensor([0] + list(s["sq"]), dtype=torch.int64).cumsum(0).to(torch.int32))
        pos.copy_(torch.tensor(s["pos"], dtype=torch.int32))
        qkv.copy_(torch.randn(T, Wd, generator=g, device=DEV).to(dtype))

    def step(kv):
        xq = eng.rope_kv_store_paged_varq(qkv, freqs, *kv, pt.table, cu, maxq, pos, W.H, W.HKV)
        return eng.attn_paged_varq_window(xq, *kv, pt.table, cu, maxq, pos, L, 1, floor, left, True, scale, True)
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
    eager = [t.clone() for t in pools]
    seen = []
    for s in steps:
        load(s)
        out.fill_(W.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = step(eager)                # eager, on pools that took the same stores
        n = sum(s["sq"])
        assert torch.isfinite(out[:n].float()).all() and out[:n].any() and torch.equal(bits(out[:n]), bits(want[:n])), s
        assert (out[n:] == W.SENTINEL).all() and all(torch.equal(bits(a), bits(e)) for a, e in zip(pools, eager))
        seen.append(out[:n].clone())
    assert not torch.equal(bits(seen[0][:1]), bits(seen[1][:1]))
    # the scheduler's rule after the second step, then NaN in every page that went back: the replay of the same step keeps its bits
    freed = 0
    before = {b: set(pt.pages(b)) for b in range(B)}
    for b, (n, p) in enumerate(zip(steps[1]["sq"], steps[1]["pos"])):
        freed += pt.release_before(b, max(0, p + n - left) & ~63)
    gone = sorted(set().union(*before.values()) - set().union(*(set(pt.pages(b)) for b in range(B))))
    assert freed == len(gone) == 3 and pt.table[1, :3].tolist() == [0, 0, 0]      # sequence 1: 302 keys, keys below 192 are dead
    for t in pools:
        t[gone] = float("nan")
    # the step once more: the same tokens at the same positions (the stores rewrite what they wrote), the table changed in place
    out.fill_(W.SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    n = sum(steps[1]["sq"])
    assert torch.isfinite(out[:n].float()).all() and torch.equal(bits(out[:n]), bits(seen[1]))
