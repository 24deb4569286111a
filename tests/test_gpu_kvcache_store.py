"""The store launch with device positions (awq_rope_kv_store_natural_pos[_fp8], csrc/awq_attn_chunk_cdna4.hip, csrc/awq_attn_kv8_cdna4.hip)
against per-sequence calls of the host-position launch, whole caches compared over a sentinel; and one captured graph of store +
attention replayed over several decode steps while the lengths advance on the device."""
import math

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_oracle as O
from tests import attn_splitkv_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape, dtype, mul):
    n = math.prod(shape)
    pat = (torch.arange(n, device=DEV) * mul + 12345) % 30011  # as 16-bit patterns: finite and positive
    if dtype == torch.uint8:
        return (pat % 251).to(torch.uint8).reshape(shape).clone()
    if dtype == torch.float32:
        return (pat.float() + 0.5).reshape(shape).clone()
    return pat.to(torch.int16).view(dtype).reshape(shape).clone()


def _table(rows, rot, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (50.0 * torch.randn(rows, rot, generator=g, device=DEV)).contiguous()


def _qkv(B, S, W, dtype, seed, strided):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if not strided:
        return torch.randn(B, S, W, generator=g, device=DEV).to(dtype)
    wide = torch.full((B, S + 2, W + 24), float("nan"), dtype=dtype, device=DEV)  # batch and row strides of its own, NaN around it
    x = wide[:, :S, 8:8 + W]
    x.copy_(torch.randn(B, S, W, generator=g, device=DEV))
    return x


H, HKV, LMAX, BC = 8, 2, 211, 6


def _positions(S):
    """(0, 37, lmax - S) are active; -1 is a finished slot, lmax - S + 1 would run over the end of the cache."""
    return (0, 37, LMAX - S, -1, LMAX - S + 1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
def test_store_pos_equals_per_sequence_host_position_calls(S, Dh, dtype):
    E = _engine()
    pos = _positions(S)
    B, W = len(pos), (H + 2 * HKV) * Dh
    rot = Dh if S == 1 else Dh // 2
    table = _table(LMAX + 20, rot, seed=S + Dh)
    qkv = _qkv(B, S, W, dtype, seed=S * 7 + Dh, strided=(S == 5))
    lens = torch.tensor(pos, dtype=torch.int32, device=DEV)
    kc0, vc0 = _sentinel((BC, LMAX, HKV, Dh), dtype, 7), _sentinel((BC, LMAX, HKV, Dh), dtype, 13)
    kc_want, vc_want = kc0.clone(), vc0.clone()
    q_want = torch.zeros(B, S, H, Dh, dtype=dtype, device=DEV)
    for b in range(3):  # the active sequences, one host-position call each
        q_want[b] = ops.rope_kv_store_natural(qkv[b:b + 1], table[pos[b]:pos[b] + S], kc_want[b:b + 1], vc_want[b:b + 1], pos[b], H, HKV)[0]
    assert not torch.equal(bits(kc_want[:3]), bits(kc0[:3]))
    for fn in (ops.rope_kv_store_natural_pos, E.rope_kv_store_natural_pos):
        kc, vc = kc0.clone(), vc0.clone()
        q_out = fn(qkv, table, kc, vc, lens, H, HKV)
        torch.cuda.synchronize()
        assert q_out.shape == (B, S, H, Dh) and q_out.is_contiguous()
        assert torch.equal(bits(q_out), bits(q_want))
        assert not q_out[3:].view(torch.int16).any()  # inactive and overflowing: a zero q
        assert torch.equal(bits(kc), bits(kc_want)) and torch.equal(bits(vc), bits(vc_want))  # the WHOLE caches
        assert torch.equal(bits(kc[3:]), bits(kc0[3:])) and torch.equal(bits(vc[3:]), bits(vc0[3:]))  # .. rows 3, 4 (and 5) untouched
    # a table that ends one row early makes the sequence at lmax - S inactive too: active means pos + S <= min(lmax, table rows)
    kc, vc = kc0.clone(), vc0.clone()
    q_out = ops.rope_kv_store_natural_pos(qkv, table[:LMAX - 1], kc, vc, lens, H, HKV)
    assert torch.equal(bits(q_out[:2]), bits(q_want[:2])) and not q_out[2:].view(torch.int16).any()
    assert torch.equal(bits(kc[:2]), bits(kc_want[:2])) and torch.equal(bits(kc[2:]), bits(kc0[2:])) and torch.equal(bits(vc[2:]), bits(vc0[2:]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
def test_store_pos_fp8_equals_per_sequence_host_position_calls_in_codes_and_scales(S, Dh, dtype):
    E = _engine()
    pos = _positions(S)
    B, W = len(pos), (H + 2 * HKV) * Dh
    rot = Dh // 2 if S == 1 else Dh
    table = _table(LMAX + 20, rot, seed=S + Dh + 1)
    qkv = _qkv(B, S, W, dtype, seed=S * 11 + Dh, strided=(S == 5))
    lens = torch.tensor(pos, dtype=torch.int32, device=DEV)
    zero = (_sentinel((BC, LMAX, HKV, Dh), torch.uint8, 7), _sentinel((BC, LMAX, HKV, Dh), torch.uint8, 13),
            _sentinel((BC, LMAX, HKV), torch.float32, 3), _sentinel((BC, LMAX, HKV), torch.float32, 5))
    want = [t.clone() for t in zero]
    q_want = torch.zeros(B, S, H, Dh, dtype=dtype, device=DEV)
    for b in range(3):
        q_want[b] = ops.rope_kv_store_natural_fp8(qkv[b:b + 1], table[pos[b]:pos[b] + S], *(t[b:b + 1] for t in want), pos[b], H, HKV)[0]
    for fn in (lambda *a: ops.rope_kv_store_natural_pos(*a[:4], a[6], a[7], a[8], k_scale=a[4], v_scale=a[5]), E.rope_kv_store_natural_pos_fp8):
        got = [t.clone() for t in zero]
        q_out = fn(qkv, table, *got, lens, H, HKV)
        torch.cuda.synchronize()
        assert torch.equal(bits(q_out), bits(q_want)) and not q_out[3:].view(torch.int16).any()
        for g, w, z in zip(got, want, zero):  # codes and scales, the whole tensors, bit for bit
            assert torch.equal(g.view(torch.uint8), w.view(torch.uint8))
            assert torch.equal(g[3:].view(torch.uint8), z[3:].view(torch.uint8))
    # q is the T cache's q
    kc, vc = torch.zeros(BC, LMAX, HKV, Dh, dtype=dtype, device=DEV), torch.zeros(BC, LMAX, HKV, Dh, dtype=dtype, device=DEV)
    assert torch.equal(bits(ops.rope_kv_store_natural_pos(qkv, table, kc, vc, lens, H, HKV)), bits(q_want))


def test_store_pos_refuses_what_it_cannot_read():
    E = _engine()
    Dh = 64
    qkv = torch.zeros(2, 1, (H + 2 * HKV) * Dh, dtype=torch.float16, device=DEV)
    table = torch.zeros(32, Dh, device=DEV)
    kc = torch.zeros(2, 32, HKV, Dh, dtype=torch.float16, device=DEV)
    lens = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):
        E.rope_kv_store_natural_pos(qkv, table, kc, kc.clone(), lens.long(), H, HKV)
    with pytest.raises(RuntimeError, match="GPU"):
        E.rope_kv_store_natural_pos(qkv, table, kc, kc.clone(), lens.cpu(), H, HKV)
    with pytest.raises(RuntimeError, match="int32"):
        E.rope_kv_store_natural_pos(qkv, table, kc, kc.clone(), lens[:1], H, HKV)
    with pytest.raises(RuntimeError, match="freqs_table"):
        E.rope_kv_store_natural_pos(qkv, table[None], kc, kc.clone(), lens, H, HKV)
    with pytest.raises(ValueError, match="int32"):
        ops.rope_kv_store_natural_pos(qkv, table, kc, kc.clone(), lens.long(), H, HKV)
    with pytest.raises(RuntimeError, match="max_seqlen_k"):
        E.attn_kvcache(torch.zeros(2, 1, H, Dh, dtype=torch.float16, device=DEV), kc, kc, lens, 33, 0, 0.125, True)
    with pytest.raises(RuntimeError, match="128"):
        E.attn_kvcache(torch.zeros(2, 33, H, Dh, dtype=torch.float16, device=DEV), kc, kc, lens, 32, 0, 0.125, True)
    assert not kc.any()


# ------------------------------------------------------------------------------------------------------------------------
# one captured graph for the decode phase
# ------------------------------------------------------------------------------------------------------------------------
def test_one_graph_replays_the_decode_steps_while_the_lengths_advance_on_the_device():
    E = _engine()
    B, Dh, L, dtype, steps = 2, 128, 320, torch.bfloat16, 6
    W = (H + 2 * HKV) * Dh
    start = (60, 130)
    table = _table(L, Dh, seed=5) * 0.02
    g = torch.Generator(device=DEV).manual_seed(17)
    mul = torch.cat([torch.full((H * Dh,), 1.5), torch.ones(HKV * Dh), torch.full((HKV * Dh,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + HKV) * Dh), torch.ones(HKV * Dh)]).to(DEV)

    def draw(*shape):
        return (torch.randn(*shape, W, generator=g, device=DEV) * mul + add).to(dtype)
    kc, vc = torch.full((B, L, HKV, Dh), float("nan"), dtype=dtype, device=DEV), torch.full((B, L, HKV, Dh), float("nan"), dtype=dtype, device=DEV)
    for b, n in enumerate(start):  # the history, one sequence at a time through the host-position launch
        ops.rope_kv_store_natural(draw(1, n), table[:n], kc[b:b + 1], vc[b:b + 1], 0, H, HKV)
    kc1, vc1 = kc[1:2].clone(), vc[1:2].clone()  # sequence 1 again, for the host-length path
    lens = torch.tensor(start, dtype=torch.int32, device=DEV)
    x = draw(B, 1)
    scale = Dh ** -0.5
    _capi.tune(attn_splitkv_chunk=64)
    try:
        assert ops.attn_kvcache_plan(B, H, HKV, Dh, 1, L) == (5, 64)

        def step():
            return E.attn_kvcache(E.rope_kv_store_natural_pos(x, table, kc, vc, lens, H, HKV), kc, vc, lens, L, 1, scale, True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream (it stores the token the first replay stores again)
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()  # q_out and the workspace come from the graph's pool
        for t in range(steps):
            x.copy_(draw(B, 1))
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            pos = [n + t for n in start]
            assert lens.tolist() == pos
            # the new entries, eagerly, with the same lengths (the store writes the same token to the same place again)
            xq = ops.rope_kv_store_natural_pos(x, table, kc, vc, lens, H, HKV)
            assert torch.equal(bits(ops.attn_kvcache(xq, kc, vc, lens, L, 1, None, True)), bits(got)), t
            # sequence 1 through the host-length path: B = 1 store, B = 1 split-KV attention
            xq1 = ops.rope_kv_store_natural(x[1:2], table[pos[1]:pos[1] + 1], kc1, vc1, pos[1], H, HKV)
            assert ops.attn_splitkv_plan(1, H, HKV, Dh, 1, pos[1] + 1, True)[0] > 1
            assert torch.equal(bits(ops.attn_splitkv(xq1, kc1[:, :pos[1] + 1], vc1[:, :pos[1] + 1], None, True)), bits(got[1:2])), t
            for b in range(B):
                n = pos[b] + 1
                ref, Aw, qk = O.attention(xq[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], None, True, stats=True)
                err = (got[b:b + 1].double() - ref).abs()
                assert not (err > S.bound(ref, Aw, qk, dtype, n, Dh, scale, 5)).any(), (t, b)
            lens += 1  # on the device, in place: the next replay reads it
        assert lens.tolist() == [n + steps for n in start] and start[0] + steps > 64 > start[0]  # sequence 0 crossed the first chunk edge
        assert torch.isnan(kc[0, start[0] + steps:]).all() and not torch.isnan(kc[0, :start[0] + steps]).any()
    finally:
        _capi.tune(attn_splitkv_chunk=0)
