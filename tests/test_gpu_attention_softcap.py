"""Soft-capped attention on packed steps on the GPU (awq_attn_varq_softcap[_kv8], awq_attn_paged_varq_softcap[_kv8]; csrc/awq_softcap.hpp):
the step of tests/attn_softcap_cases.py -- the windowed step: H 8 / Hkv 2, bound 512, chunk forced to 64, pages of 64 / 128 keys.

    1. every row within attn_softcap_oracle.bound of the float64 oracle: caps 2 and 50, lefts 100 and 511, under the rule's routes
       (split_min_keys 128) and with every short sequence forced onto the split pair (split_min_keys 1), dense and both page sizes, T and
       FP8, every (dtype, Dh); once with the scale 144 ** -0.5
    2. softcap = 0 returns the bits of attn_varq_window
    3. paged equals dense on the gathered keys, bit for bit
    4. FP8 equals T on the dequantised caches, bit for bit
    5. a sequence's rows equal the same call on that sequence alone, bit for bit, on the route written down by hand
    6. NaN below every first tile -- and the NaN the step keeps in every cache row that holds no key -- changes nothing
    7. one captured graph replays two steps with the lengths advanced on the device

Measured figures of test 1 are printed before they are asserted (the worst |err| / bound of every call)."""
import os
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_softcap_cases as C
from tests import attn_softcap_oracle as O
from tests import attn_window_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DATA, _REF = {}, {}
LAYOUTS = [0, 64, 128]
IDS = lambda x: str(x).replace("torch.", "")
CAPS = (2.0, 50.0)
FORMS = [(ps, fp8) for ps in LAYOUTS for fp8 in (False, True)]      # (page size or 0 for dense, FP8 cache)


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def knobs():
    """The split chunk forced to 64 keys and the one-pass q tile to 128 rows, as in the window's tests.  Both are restored afterwards."""
    had = os.environ.get("AWQ_TUNING")
    _capi.tune(attn_splitkv_chunk=C.CHUNK, attn_prefill_rows=128)
    yield lambda rows: _capi.tune(attn_prefill_rows=rows)
    _capi.tune(attn_splitkv_chunk=0, attn_prefill_rows=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def _layout(st, k_cache, v_cache, ps):
    """(k, v, table) on the GPU: the caches, or the shuffled pages of them."""
    if not ps:
        return k_cache.to(DEV), v_cache.to(DEV), None
    view = SimpleNamespace(held=st.held, Dh=st.Dh, dtype=st.dtype, k_cache=k_cache, v_cache=v_cache)
    pool = W.S.Pool(view, ps)
    table = pool.table_full.to(DEV)[:, :pool.pps]
    assert table.stride(0) > table.shape[1]
    return pool.k_pool.to(DEV), pool.v_pool.to(DEV), table


def _pack(st, k, v, table):
    kq, ks = ops.kv8_quant(k.nan_to_num(0.0))
    vq, vs = ops.kv8_quant(v.nan_to_num(0.0))
    return SimpleNamespace(st=st, q=st.q.to(DEV), k=k, v=v, kq=kq, vq=vq, ks=ks, vs=vs, table=table, cu=st.cu_seqlens_q.to(DEV),
                           lens=st.seqlens_k(True).to(DEV))


def _data(dtype, Dh, ps):
    """The step's tensors on the GPU, built once per (dtype, Dh, layout) and never written."""
    key = (dtype, Dh, ps)
    if key not in _DATA:
        st = _DATA.get((dtype, Dh)) or _DATA.setdefault((dtype, Dh), C.Step(dtype, Dh))
        _DATA[key] = _pack(st, *_layout(st, st.k_cache, st.v_cache, ps))
    return _DATA[key]


def _reference(dtype, Dh, fp8, left, cap, scale):
    """Per active sequence (ref, bound), float64 on the CPU, computed once per key and shared."""
    key = (dtype, Dh, fp8, left, cap, scale)
    if key not in _REF:
        d = _data(dtype, Dh, 0)
        st = d.st
        k, v = (ops.kv8_dequant(d.kq, d.ks, dtype).cpu(), ops.kv8_dequant(d.vq, d.vs, dtype).cpu()) if fp8 else (st.k_cache, st.v_cache)
        out = {}
        for b, (n, h) in enumerate(C.STEP):
            if C.active_rows(b):
                ref, A, qk = O.attention(*st.seq(b, k, v), left, cap, scale=scale, stats=True)
                out[b] = (ref[0], O.bound(ref, A, qk, dtype, h + n, Dh, scale, cap)[0])
        _REF[key] = out
    return _REF[key]


def _sentinel(d):
    return torch.full((d.st.total_q, C.H, d.st.Dh), C.SENTINEL, dtype=d.st.dtype, device=DEV)


def _run(d, fp8, left, cap, floor=C.SPLIT_MIN_KEYS, split_q=C.SPLIT_SEQLEN_Q, scale=None, window=False):
    kv = (d.kq, d.vq) if fp8 else (d.k, d.v)
    kw = dict(k_scale=d.ks, v_scale=d.vs) if fp8 else {}
    kw.update(block_table=d.table, out=_sentinel(d), softmax_scale=scale)
    if window:         # the call without a cap
        return ops.attn_varq_window(d.q, *kv, d.cu, C.MAX_Q, d.lens, C.BOUND, left, split_q, floor, **kw)
    return ops.attn_varq_softcap(d.q, *kv, d.cu, C.MAX_Q, d.lens, C.BOUND, cap, left, split_q, floor, **kw)


def _check_against_oracle(d, fp8, out, left, cap, scale, what):
    st = d.st
    n_rows = st.cu[-1]
    refs = _reference(st.dtype, st.Dh, fp8, left, cap, scale)
    assert torch.isfinite(out.float()).all(), (what, "a NaN: a row that holds no key, or a padding row, was read")
    o = out.double().cpu()
    worst = {}
    for b, (n, h) in enumerate(C.STEP):
        sl = slice(st.cu[b], st.cu[b + 1])
        if b in refs:
            ref, bound = refs[b]
            worst[b] = float(((o[sl] - ref).abs() / bound).max())
        else:
            assert not out[sl].any(), (what, left, b, "an inactive slot's rows are zeros")
    at = max(worst, key=worst.get)                    # one figure a call, printed before it is asserted: the sequence nearest its bound
    what = f"{what} {'fp8' if fp8 else 'T'} {'ps %d' % d.k.shape[1] if d.table is not None else 'dense'}"
    print(f"{what} cap {cap} left {left}: worst |err| / bound = {worst[at]:.3f} (seq {at} {C.STEP[at]})")
    assert all(w <= 1.0 for w in worst.values()), (what, cap, left, worst)
    assert (out[n_rows:] == C.SENTINEL).all() and out[n_rows:].shape[0] == C.PAD_ROWS


# ------------------------------------------------------------------------------------------------------------------------
# 1. the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", C.COMBOS, ids=IDS)
def test_every_row_is_within_the_bound_of_the_oracle(dtype, Dh, knobs):
    for ps, fp8 in FORMS:                  # dense and both page sizes, T and FP8: one case a (dtype, Dh), the forms inside it
        _every_row_is_within_the_bound(dtype, Dh, ps, fp8, knobs)


def _every_row_is_within_the_bound(dtype, Dh, ps, fp8, knobs):
    knobs(128)
    d = _data(dtype, Dh, ps)
    scale = Dh ** -0.5
    for cap in CAPS:
        for left in C.LEFTS:
            assert W.routes(left) == W.TAKEN[left]
            _check_against_oracle(d, fp8, _run(d, fp8, left, cap), left, cap, scale, "rule")
            _check_against_oracle(d, fp8, _run(d, fp8, left, cap, floor=1), left, cap, scale, "forced")    # every short sequence on the split pair
    knobs(64)                                                                                              # the 64-row q tile: two waves
    _check_against_oracle(d, fp8, _run(d, fp8, 100, 2.0), 100, 2.0, scale, "rows64")
    if not ps and not fp8:                                                                                 # Gemma-2-27B's scale, once per (dtype, Dh)
        g = C.GEMMA2_SCALE
        for floor in (C.SPLIT_MIN_KEYS, 1):
            _check_against_oracle(d, fp8, _run(d, fp8, 511, 50.0, floor=floor, scale=g), 511, 50.0, g, "scale144")
        capped = _run(d, fp8, 511, 50.0, scale=g)
        assert not torch.equal(bits(capped), bits(_run(d, fp8, 511, 50.0)))                                # the scale is taken


# ------------------------------------------------------------------------------------------------------------------------
# 2. no cap
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", C.COMBOS[:2], ids=IDS)
def test_softcap_0_returns_the_bits_of_the_windowed_call(dtype, Dh, knobs):
    for ps, fp8 in FORMS:
        _softcap_0_returns_the_bits_of_the_windowed_call(dtype, Dh, ps, fp8)


def _softcap_0_returns_the_bits_of_the_windowed_call(dtype, Dh, ps, fp8):
    d = _data(dtype, Dh, ps)
    for floor, split_q in ((C.SPLIT_MIN_KEYS, C.SPLIT_SEQLEN_Q), (1, C.SPLIT_SEQLEN_Q), (C.SPLIT_MIN_KEYS, 0)):
        for left in C.LEFTS:
            plain = _run(d, fp8, left, None, floor, split_q, window=True)
            assert plain[:d.st.cu[-1]].any()
            assert torch.equal(bits(_run(d, fp8, left, 0.0, floor, split_q)), bits(plain)), (ps, fp8, floor, split_q, left)
            assert not torch.equal(bits(_run(d, fp8, left, 50.0, floor, split_q)), bits(plain)), (ps, fp8, floor, split_q, left)
    # window_left None is max_seqlen_k - 1: a window that hides nothing
    kv = (d.kq, d.vq) if fp8 else (d.k, d.v)
    kw = dict(k_scale=d.ks, v_scale=d.vs) if fp8 else {}
    glob = ops.attn_varq_softcap(d.q, *kv, d.cu, C.MAX_Q, d.lens, C.BOUND, 50.0, None, C.SPLIT_SEQLEN_Q, C.SPLIT_MIN_KEYS, block_table=d.table,
                                 out=_sentinel(d), **kw)
    assert torch.equal(bits(glob), bits(_run(d, fp8, C.BOUND - 1, 50.0))) and torch.equal(bits(glob), bits(_run(d, fp8, 10 ** 6, 50.0))), (ps, fp8)


# ------------------------------------------------------------------------------------------------------------------------
# 3. / 4. the layouts and the cache formats
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", C.COMBOS, ids=IDS)
def test_paged_equals_dense_bit_for_bit(dtype, Dh, knobs):
    dense = _data(dtype, Dh, 0)
    for fp8 in (False, True):
        for cap, left, floor in ((2.0, 100, C.SPLIT_MIN_KEYS), (50.0, 511, C.SPLIT_MIN_KEYS), (50.0, 100, 1)):
            want = _run(dense, fp8, left, cap, floor)
            assert want[:dense.st.cu[-1]].any()
            for ps in C.PAGE_SIZES:
                assert torch.equal(bits(_run(_data(dtype, Dh, ps), fp8, left, cap, floor)), bits(want)), (fp8, cap, left, floor, ps)


@pytest.mark.parametrize("dtype,Dh", C.COMBOS, ids=IDS)
def test_fp8_equals_T_on_the_dequantised_caches_bit_for_bit(dtype, Dh, knobs):
    for ps in LAYOUTS:
        d = _data(dtype, Dh, ps)
        deq = SimpleNamespace(**vars(d))
        deq.k, deq.v = ops.kv8_dequant(d.kq, d.ks, dtype), ops.kv8_dequant(d.vq, d.vs, dtype)
        for cap, left, floor in ((2.0, 100, C.SPLIT_MIN_KEYS), (50.0, 511, C.SPLIT_MIN_KEYS), (50.0, 100, 1)):
            got = _run(d, True, left, cap, floor)
            assert got[:d.st.cu[-1]].any() and torch.equal(bits(got), bits(_run(deq, False, left, cap, floor))), (ps, cap, left, floor)


# ------------------------------------------------------------------------------------------------------------------------
# 5. batch independence
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", C.COMBOS[:2], ids=IDS)
def test_every_sequence_equals_the_call_on_that_sequence_alone(dtype, Dh, knobs):
    for ps, fp8 in FORMS:
        _every_sequence_equals_the_call_on_that_sequence_alone(dtype, Dh, ps, fp8)


def _every_sequence_equals_the_call_on_that_sequence_alone(dtype, Dh, ps, fp8):
    d = _data(dtype, Dh, ps)
    st = d.st
    kv = (d.kq, d.vq, d.ks, d.vs) if fp8 else (d.k, d.v)
    for cap, left in ((2.0, 100), (50.0, 511)):
        out = _run(d, fp8, left, cap)
        for b, (n, h) in enumerate(C.STEP):
            if not n:
                continue
            sl = slice(st.cu[b], st.cu[b + 1])
            one = kv if ps else tuple(t[b:b + 1] for t in kv)
            cu = torch.tensor([0, n], dtype=torch.int32, device=DEV)
            taken = W.TAKEN[left][b]
            # alone, on the route written down: the split pair whatever the keys (floor 1), or the one-pass kernel alone (split_seqlen_q 0)
            alone = ops.attn_varq_softcap(d.q[sl], *one[:2], cu, C.MAX_Q, d.lens[b:b + 1], C.BOUND, cap, left, C.SPLIT_SEQLEN_Q if taken else 0, 1,
                                          block_table=d.table[b:b + 1] if ps else None, **(dict(k_scale=one[2], v_scale=one[3]) if fp8 else {}))
            assert torch.equal(bits(out[sl]), bits(alone)), (ps, fp8, cap, left, b, C.STEP[b], taken)
    eng = _engine()                       # the engine binding gives the bits of ops
    name = "attn" + ("_paged" if ps else "") + "_varq_softcap" + ("_kv8" if fp8 else "")
    where = (*kv, *((d.table,) if ps else ()))
    e_out = getattr(eng, name)(d.q, *where, d.cu, C.MAX_Q, d.lens, C.BOUND, C.SPLIT_SEQLEN_Q, C.SPLIT_MIN_KEYS, 511, 50.0, True, Dh ** -0.5, True,
                               _sentinel(d))
    assert torch.equal(bits(e_out), bits(out)), (ps, fp8)


# ------------------------------------------------------------------------------------------------------------------------
# 6. dead keys
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", C.COMBOS[:2], ids=IDS)
def test_nan_below_every_first_tile_and_in_every_unheld_row_changes_nothing(dtype, Dh, knobs):
    for ps, fp8 in FORMS:
        _nan_below_every_first_tile_changes_nothing(dtype, Dh, ps, fp8)


def _nan_below_every_first_tile_changes_nothing(dtype, Dh, ps, fp8):
    clean = _data(dtype, Dh, ps)
    st = clean.st
    nan = float("nan")
    for b, n in enumerate(st.held):                                   # the step itself: NaN in every cache row that holds no key
        assert torch.isnan(st.k_cache[b, n:].float()).all() and torch.isnan(st.v_cache[b, n:].float()).all()
    left = 100
    k, v = st.k_cache.clone(), st.v_cache.clone()
    dead = 0
    for b, (n, h) in enumerate(C.STEP):
        if C.active_rows(b):
            a = W.anchor(b, left)
            k[b, :a], v[b, :a] = nan, nan
            dead += a
    assert dead > 0
    d = _pack(st, *_layout(st, k, v, ps))
    if fp8:                                # NaN codes (e4m3fn 0x7F) and NaN scales wherever the T cache holds NaN
        hole = torch.isnan(d.k.float()).all(-1)
        for codes, scales in ((d.kq, d.ks), (d.vq, d.vs)):
            codes.view(torch.uint8)[hole] = 0x7F
            scales[hole] = nan
    if ps:                                 # every table entry below the first tile names the all-NaN poison page
        pool = W.S.Pool(SimpleNamespace(held=st.held, Dh=st.Dh, dtype=st.dtype, k_cache=k, v_cache=v), ps)
        table = d.table.clone()
        for b, (n, h) in enumerate(C.STEP):
            if C.active_rows(b):
                table[b, :W.anchor(b, left) // ps] = pool.poison
        assert torch.isnan(d.k[pool.poison].float()).all()
        d.table = table
    for cap in CAPS:
        for floor in (C.SPLIT_MIN_KEYS, 1):
            want = _run(clean, fp8, left, cap, floor)
            got = _run(d, fp8, left, cap, floor)
            assert torch.isfinite(got.float()).all() and torch.equal(bits(got), bits(want)), (ps, fp8, cap, floor)


# ------------------------------------------------------------------------------------------------------------------------
# 7. one graph, two steps
# ------------------------------------------------------------------------------------------------------------------------
def test_one_graph_replays_two_steps_with_the_lengths_advanced_on_the_device(knobs):
    dtype, Dh, B, L, floor, left, cap = torch.bfloat16, 128, 3, 512, 64, 100, 50.0
    scale = C.GEMMA2_SCALE
    g = torch.Generator(device=DEV).manual_seed(53)
    kc = torch.randn(B, L, C.HKV, Dh, generator=g, device=DEV).to(dtype)
    vc = torch.randn(B, L, C.HKV, Dh, generator=g, device=DEV).to(dtype)
    q = (1.5 * torch.randn(B, C.H, Dh, generator=g, device=DEV)).to(dtype)
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    lens = torch.tensor([300, 40, 199], dtype=torch.int32, device=DEV)        # keys_b = 101, 41, 101: the split pair, one-pass, the pair
    out = torch.empty(B, C.H, Dh, dtype=dtype, device=DEV)

    def step():
        ops.attn_varq_softcap(q, kc, vc, cu, 1, lens, L, cap, left, 1, floor, softmax_scale=scale, out=out)
        lens.add_(1)                                                          # the next step's lengths, formed on the device
    first = lens.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    lens.copy_(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    lens.copy_(first)
    seen = []
    for i in range(2):
        now = lens.clone()
        out.fill_(C.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lens, now + 1)
        want = ops.attn_varq_softcap(q, kc, vc, cu, 1, now, L, cap, left, 1, floor, softmax_scale=scale)
        assert torch.isfinite(out.float()).all() and out.any() and torch.equal(bits(out), bits(want)), i
        seen.append(out.clone())
    assert not torch.equal(bits(seen[0]), bits(seen[1]))
    for b in range(B):                                                        # and the second step is the oracle's
        n = int(first[b]) + 2
        ref, A, qk = O.attention(q[b:b + 1, None].cpu(), kc[b:b + 1, :n].cpu(), vc[b:b + 1, :n].cpu(), left, cap, scale=scale, stats=True)
        err = (seen[1][b].double().cpu() - ref[0, 0]).abs()
        assert bool((err <= O.bound(ref, A, qk, dtype, n, Dh, scale, cap)[0, 0]).all()), b
