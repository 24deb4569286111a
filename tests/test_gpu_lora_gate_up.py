"""gpu: multi-LoRA on QuantLlamaMLP's gate / up pair (awq_lora_expand_gate_up, ops.lora_apply_gate_up, LoRAGateUp / attach_lora_mlp).  Two references
at once: the on-device composition of the existing launches (de-interleave -> ops.lora_apply with slice_end = (F, 2F) -> ops.silu_mul), which the
fused expand must equal in every bit, and the float64 oracle's accepted codes (tests/lora_gate_up_oracle.py), whose mutants the host tests reject.
Rows outside the contract: NaN in their x, in their y2, throughout the workspace and in unnamed pool slots; a sentinel in their h."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from llm_awq_amd import load_engine, ops, synth
from llm_awq_amd.lora import LoRAGateUp, LoRALinear, LoRAPool, attach_lora, attach_lora_mlp
from tests import lora_gate_up_oracle as G
from tests import lora_oracle as L
from tests import tail_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = G.gpu_shapes()
shape_id = lambda s: "k%d-r%d-f%d" % s
bits = L.bits


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _nan_ws(case):
    return torch.full((ops.lora_workspace_bytes(case["total_q"], case["K"], case["R"], 2) // 4,), float("nan"), dtype=torch.float32, device=DEV)


def _run(case, max_sq=None):
    """ops.lora_apply_gate_up on a built case: x is the strided view of its storage (ldx = K + 8, NaN in the gap), the workspace is NaN beforehand,
    h holds the sentinel"""
    h = _dev(case["h_init"]).clone()
    out = ops.lora_apply_gate_up(_dev(case["x_store"])[:, :case["K"]], _dev(case["y2"]), _dev(case["a_pool"]), _dev(case["b_pool"]), _dev(case["scaling"]),
                                 _dev(case["ids"]), _dev(case["cu"]), case["max_sq"] if max_sq is None else max_sq, _nan_ws(case), h)
    assert out is h
    return h.cpu()


def _compose_dev(x, y2, a_pool, b_pool, scaling, ids, cu, max_sq, ws=None):
    """the composition of the existing launches on device tensors: de-interleave, lora_apply on [gate | up] with one slice per projection, silu_mul.
    awq_lora_expand takes slice ends in units of 16 columns, and F = 8, 24, 136 are 8 short of one: there each slice is padded to Fp = 16 ceil(F / 16)
    columns (zero base columns, zero rows of B) and slice_end = (Fp, 2 Fp).  A column's bits depend on hT and on its own row of B alone (one MFMA
    column), so the F real columns of each slice carry the bits the contract states for them."""
    F = y2.shape[1] // 2
    Fp = -(-F // 16) * 16
    stacked = G.deinterleave(y2)
    if Fp != F:
        zy = torch.zeros(y2.shape[0], Fp - F, dtype=y2.dtype, device=y2.device)
        zb = torch.zeros(b_pool.shape[0], Fp - F, b_pool.shape[2], dtype=b_pool.dtype, device=b_pool.device)
        stacked = torch.cat([stacked[:, :F], zy, stacked[:, F:], zy], 1)
        b_pool = torch.cat([b_pool[:, :F], zb, b_pool[:, F:], zb], 1).contiguous()
    stacked = stacked.contiguous()
    ops.lora_apply(x, stacked, a_pool, b_pool, scaling, ids, (Fp, 2 * Fp), cu, max_sq, ws)
    return ops.silu_mul(stacked[:, :F].contiguous(), stacked[:, Fp:Fp + F].contiguous())


def _compose(case):
    return _compose_dev(_dev(case["x_store"])[:, :case["K"]], _dev(case["y2"]), _dev(case["a_pool"]), _dev(case["b_pool"]), _dev(case["scaling"]),
                        _dev(case["ids"]), _dev(case["cu"]), case["max_sq"], _nan_ws(case)).cpu()


def _check(case, h, oracle=True):
    """written rows: the composition's bits (and inside the oracle's accepted codes); every other row: the sentinel"""
    w = torch.from_numpy(case["active"])
    assert torch.equal(bits(h)[~w], bits(case["h_init"])[~w]), "a row outside the contract was written"
    assert torch.equal(bits(h)[w], bits(_compose(case))[w]), "not the bits of lora_apply + silu_mul"
    assert not torch.equal(bits(h)[w], bits(case["h_init"])[w])
    if oracle:
        G.check(case, h)


@functools.lru_cache(maxsize=None)
def _packed_lattice(shape, dtype_name, scale_m=1):
    return G.build_lattice(*shape, dtype_name, scale_m=scale_m, **G.PACKED)


@pytest.mark.parametrize("B", [1, 2, 17])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lattice_decode_rows(shape, dtype_name, B):
    """the rectangular form, one row per sequence.  With B < 3 some pool slot is named by nobody and holds NaN."""
    case = G.build_lattice(*shape, dtype_name, rect=(B, 1))
    _check(case, _run(case))


@pytest.mark.parametrize("scale_m", [1, 3], ids=["pow2", "x1.5"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lattice_packed_step_is_exact_untouched_and_stable(shape, dtype_name, scale_m):
    """Sq = [1, 0, 0, 17, 3, 16, 33, 1] with ids [0, -1, 2, 1, 0, 2, 1, S] and four padding rows: the last sequence is active WITHOUT an adapter (the
    plain tail), the padding rows and nothing else keep the sentinel.  The same under a max_seqlen_q eight times too loose, and three runs give the
    same bits."""
    case = _packed_lattice(shape, dtype_name, scale_m)
    got = _run(case)
    _check(case, got)
    plain = torch.from_numpy(case["plain"])
    want = ops.silu_mul(*(t.contiguous() for t in G.deinterleave(_dev(case["y2"])[plain]).split(case["F"], 1))).cpu()
    assert plain.sum() == 1 and torch.equal(bits(got)[plain], bits(want))          # no adapter: the tail on the pair itself
    assert torch.equal(bits(_run(case, max_sq=8 * case["max_sq"])), bits(got))
    assert torch.equal(bits(_run(case)), bits(got)) and torch.equal(bits(_run(case)), bits(got))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_an_inactive_sequence_keeps_its_sentinel(dtype_name):
    """max_seqlen_q = 17 makes the 33-row sequence inactive: its rows of h keep the sentinel (their y2 is NaN and is not read)"""
    case = G.build_lattice(*SHAPES[4], dtype_name, max_sq=17, **G.PACKED)
    assert not case["active"][37:70].any() and case["active"][20] and torch.isnan(case["y2"][37:70].float()).all()
    _check(case, _run(case))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5], SHAPES[7]], ids=shape_id)
def test_a_rows_bits_do_not_depend_on_its_batch(shape, dtype_name):
    """every sequence of the packed step, run alone through the rectangular form, gives the same bits for its rows"""
    case = _packed_lattice(shape, dtype_name)
    K = case["K"]
    got = _run(case)
    x, y2 = _dev(case["x_store"])[:, :K], _dev(case["y2"])
    pools = [_dev(case[n]) for n in ("a_pool", "b_pool", "scaling")]
    seen = 0
    for b, sq in enumerate(G.PACKED_SQ):
        lo = int(case["cu"][b])
        if sq == 0:
            continue
        h = ops.lora_apply_gate_up(x[lo:lo + sq], y2[lo:lo + sq].contiguous(), *pools, _dev(case["ids"][b:b + 1]), None, sq)
        assert torch.equal(bits(h), bits(got[lo:lo + sq])), b
        seen += 1
    assert seen == 6      # five sequences on an adapter, one without


RANDOM_SHAPES = [(1024, 64, 136), (192, 16, 24), (L.find_uneven_k(L.plan, 32, 2), 32, 8), (4096, 64, 8)]


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=shape_id)
def test_random_inputs_equal_the_composition(shape, dtype_name):
    """no tolerance: the composition's own distance to float64 is covered by tests/test_gpu_lora.py"""
    case = G.build_random(*shape, dtype_name, **G.PACKED)
    _check(case, _run(case), oracle=False)
    case = G.build_random(*shape, dtype_name, rect=(5, 1))
    _check(case, _run(case), oracle=False)


def test_ops_and_the_engine_entry_agree():
    eng = load_engine()
    case = _packed_lattice(SHAPES[1], "bf16")
    K, R = case["K"], case["R"]
    x, y2, ids, cu = _dev(case["x_store"])[:, :K], _dev(case["y2"]), _dev(case["ids"]), _dev(case["cu"])
    a_pool, b_pool, scaling = (_dev(case[n]) for n in ("a_pool", "b_pool", "scaling"))
    ws = ops.lora_shrink(x, a_pool, ids, R, cu, case["max_sq"])
    want = _run(case)
    h = _dev(case["h_init"]).clone()
    assert eng.lora_expand_gate_up(ws, b_pool, scaling, ids, y2, K, h, cu, case["max_sq"]).data_ptr() == h.data_ptr()
    assert torch.equal(bits(h), bits(want))
    w = torch.from_numpy(case["active"])
    fresh = eng.lora_expand_gate_up(ws, b_pool, scaling, ids, y2, K, None, cu, case["max_sq"])
    assert tuple(fresh.shape) == (case["total_q"], case["F"]) and torch.equal(bits(fresh)[w], bits(want)[w])
    h2 = ops.lora_expand_gate_up(ws, b_pool, scaling, ids, y2, K, None, cu, case["max_sq"])
    assert torch.equal(bits(h2)[w], bits(want)[w])


def test_one_graph_replays_changed_ids_lengths_and_adapters():
    """shrink + the fused expand captured once; each replay equals the eager call on the state it finds"""
    K, R, F, S = 192, 32, 24, 3
    T = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    cu0, total_q = L.layout(G.PACKED_SQ, G.PACKED_PAD)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, y2 = rnd(total_q, K).to(T).to(DEV), rnd(total_q, 2 * F).to(T).to(DEV)
    a_pool, b_pool = (rnd(S, 2 * R, K) / K ** 0.5).to(T).to(DEV), (0.05 * rnd(S, 2 * F, R)).to(T).to(DEV)
    scaling = torch.tensor([2.0, 0.5, 1.0], device=DEV)
    ids, cu = _dev(np.array(G.PACKED_IDS, np.int32)), _dev(cu0)
    max_sq = max(G.PACKED_SQ)
    ws = torch.empty(ops.lora_workspace_bytes(total_q, K, R, 2) // 4, dtype=torch.float32, device=DEV)
    sentinel = _dev(G._sentinel(total_q, F, T))
    out = sentinel.clone()
    call = lambda h: ops.lora_apply_gate_up(x, y2, a_pool, b_pool, scaling, ids, cu, max_sq, ws, h)
    first = call(sentinel.clone()).clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(first)) and not torch.equal(bits(first), bits(sentinel))
    seen = [bits(first)]

    def step(change):
        change()
        out.copy_(sentinel)
        graph.replay()
        got = out.clone()
        want = call(sentinel.clone())
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want))
        assert all(not torch.equal(bits(got), s) for s in seen), "the change was not seen"
        seen.append(bits(got))

    step(lambda: ids.copy_(_dev(np.array([2, 0, 0, 0, -1, 1, 2, 1], np.int32))))
    step(lambda: cu.copy_(_dev(L.layout((4, 16, 0, 1, 33, 0, 2, 15), 0)[0])))

    def load():      # a newly loaded adapter: slot 2 rewritten in place
        a_pool[2].copy_((rnd(2 * R, K) / K ** 0.5).to(T))
        b_pool[2].copy_((0.05 * rnd(2 * F, R)).to(T))
        scaling[2] = 4.0
    step(load)


def _wq(K, N, dtype, seed):
    from llm_awq_amd.qmodule import WQLinear
    c = synth.random_wq(K, N, dtype=dtype, device=DEV, seed=seed, keep_q=False)
    m = WQLinear(4, 128, K, N, False, DEV, dtype=dtype)
    m.load_state_dict(dict(qweight=c["qweight"], scales=c["scales"], scaled_zeros=c["scaled_zeros"]))
    return m


def _mlp(K, F, dtype, seed):
    from llm_awq_amd.fused_mlp import QuantLlamaMLP
    return QuantLlamaMLP(_wq(K, F, dtype, seed), _wq(F, K, dtype, seed + 1), _wq(K, F, dtype, seed + 2))


def _unfused(mlp, x):
    c4, s, z, szp, szh = mlp._fused
    return load_engine().forward_cdna4(x, c4, s, z, szp, None, szh)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_lora_gate_up_over_a_synthetic_mlp(dtype_name):
    K, R, F = 256, 16, 384
    T = L.DTYPES[dtype_name]
    case = G.build_random(K, R, F, dtype_name, **G.PACKED)
    mlp = _mlp(K, F, T, 21)
    pool = LoRAPool(case["S"], R, T, DEV)
    gu = LoRAGateUp(mlp, pool)
    g = torch.Generator().manual_seed(3)
    for slot, r in enumerate((16, 5, 8)):      # through load_adapter: rank padding, and slot 1 targets up_proj only
        t = {"gate_proj": (torch.randn(r, K, generator=g) / 16, 0.05 * torch.randn(F, r, generator=g)),
             "up_proj": (torch.randn(r, K, generator=g) / 16, 0.05 * torch.randn(F, r, generator=g))}
        if slot == 1:
            del t["gate_proj"]
        gu.load_adapter(slot, t, alpha=2 * r, rank=r)
    x = torch.nan_to_num(_dev(case["x_store"])[:, :K]).contiguous()
    plain = mlp(x)
    assert torch.equal(bits(gu(x)), bits(plain))                                        # no batch set: the fused launch, untouched
    ids, cu = _dev(case["ids"]), _dev(case["cu"])
    pool.set_batch(ids, cu, case["max_sq"])
    got = gu(x)
    h = _compose_dev(x, _unfused(mlp, x), gu.a_pool, gu.b_pool, gu.scaling, ids, cu, case["max_sq"])
    w = torch.from_numpy(case["active"])
    assert torch.equal(bits(gu.gate_up(x))[w], bits(h)[w])
    assert torch.equal(bits(got)[w], bits(mlp.down_proj(h))[w]) and not torch.equal(bits(got)[w], bits(plain)[w])
    assert tuple(got.shape) == tuple(plain.shape) and torch.isfinite(got[w].float()).all()
    x3 = x.view(1, *x.shape)                                                            # a leading batch dimension, as a model passes it
    assert torch.equal(bits(gu(x3))[0, w], bits(got)[w])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_rows_without_an_adapter_equal_the_fused_launch_where_the_base_sums_are_exact(dtype_name):
    """selector weights (tail_oracle.selector_case): gate' = x[2 j], up' = x[2 j + 1] exactly in any summation order, so the unfused launch + plain
    tail and the fused launch must give the same bits"""
    from llm_awq_amd.fused_mlp import QuantLlamaMLP
    from llm_awq_amd.qmodule import WQLinear, pack_intweight
    K, F, R = 256, 128, 16
    T = L.DTYPES[dtype_name]
    sc = TO.selector_case(K, F, T)

    def proj(c):
        m = WQLinear(4, 128, K, F, False, DEV, dtype=T)
        m.qweight, m.scales, m.scaled_zeros = pack_intweight(torch.from_numpy(c["q"]).to(DEV)), c["scales"].to(DEV), c["scaled_zeros"].to(DEV)
        return m

    mlp = QuantLlamaMLP(proj(sc["gate"]), _wq(F, K, T, 31), proj(sc["up"]))
    pool = LoRAPool(2, R, T, DEV)
    gu = LoRAGateUp(mlp, pool)
    g = torch.Generator().manual_seed(4)
    gu.load_adapter(0, {"gate_proj": (torch.randn(R, K, generator=g) / 16, torch.randn(F, R, generator=g)),
                        "up_proj": (torch.randn(R, K, generator=g) / 16, torch.randn(F, R, generator=g))}, alpha=R, rank=R)
    cu_np, total_q = L.layout(G.PACKED_SQ, G.PACKED_PAD)
    x = (2 * torch.randn(total_q, K, generator=g)).to(T).to(DEV)
    fused = mlp.our_llama_mlp(x)
    ids = np.array([-1, 0, 0, 5, 0, -1, 2, 0], np.int32)      # slots 0 .. 1: ids 5 and 2 name nobody
    pool.set_batch(_dev(ids), _dev(cu_np), max(G.PACKED_SQ))
    h = gu.gate_up(x)
    slot = L.row_slots(ids, cu_np, len(ids), total_q, max(G.PACKED_SQ), 2)
    live = L.owners(cu_np, len(ids), total_q, max(G.PACKED_SQ)) >= 0
    plain, served = torch.from_numpy(live & (slot < 0)), torch.from_numpy(slot >= 0)
    assert plain.sum() == 1 + 17 + 16 + 33 and served.sum() == 3 + 1
    assert torch.equal(bits(h)[plain], bits(fused)[plain])
    assert not torch.equal(bits(h)[served], bits(fused)[served])
    assert torch.equal(bits(gu(x))[plain], bits(mlp(x))[plain])                        # ... and through down_proj


def test_attach_lora_mlp_and_attach_lora_inside_one_block_on_a_packed_step():
    """a block's attention (forward_packed) and MLP adapted on one pool: the MLP inside the step is the composition on the same input, and its
    down_proj is the LoRALinear attach_lora made"""
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    H, HKV, DH, LEN, F = 4, 2, 64, 128, 384
    hid, T = H * DH, torch.bfloat16
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=hid, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=LEN)
    sq = G.PACKED_SQ
    B = len(sq)
    block = torch.nn.Module()
    block.self_attn = QuantLlamaAttentionFused(hid, H, LEN, _wq(hid, (H + 2 * HKV) * DH, T, 11), _wq(hid, hid, T, 12), DEV, args, max_batch_size=B,
                                               kv_layout="natural")
    block.mlp = _mlp(hid, F, T, 41)
    inner = block.mlp
    pool = LoRAPool(3, 16, T, DEV)
    done = attach_lora(block, pool)
    assert sorted(done) == ["mlp.down_proj", "self_attn.o_proj", "self_attn.qkv_proj"]
    done_mlp = attach_lora_mlp(block, pool)
    assert sorted(done_mlp) == ["mlp"] and isinstance(block.mlp, LoRAGateUp) and inner.down_proj is done["mlp.down_proj"]
    assert isinstance(block.mlp.down_proj, LoRALinear)
    g = torch.Generator().manual_seed(9)
    pair = lambda n, k: (torch.randn(8, k, generator=g) / 16, 0.05 * torch.randn(n, 8, generator=g))
    for slot in range(3):
        pool.load_adapter(slot, {"self_attn.qkv_proj": [pair(w, hid) for w in (256, 128, 128)], "self_attn.o_proj": pair(hid, hid),
                                 "mlp": {"gate_proj": pair(F, hid), "up_proj": pair(F, hid)}, "mlp.down_proj": pair(hid, F)}, alpha=16, rank=8)
    inv = 1.0 / (10000.0 ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(LEN, device=DEV).float(), inv)
    freqs = torch.cat([f, f], -1).contiguous()
    cu_np, total_q = L.layout(sq, G.PACKED_PAD)
    cu, pos = _dev(cu_np), torch.zeros(B, dtype=torch.int32, device=DEV)
    x = (0.5 * torch.randn(1, total_q, hid, generator=g)).to(T).to(DEV)
    ids = _dev(np.array(G.PACKED_IDS, np.int32))
    pool.set_batch(ids, cu, max(sq))
    live = torch.from_numpy(L.owners(cu_np, B, total_q, max(sq)) >= 0)
    a = block.self_attn.forward_packed(x, pos, freqs, cu, max(sq))
    a = torch.where(live[None, :, None].to(DEV), a, torch.zeros_like(a))      # (the attention leaves the padding rows of its output unwritten)
    got = block.mlp(a)
    a2 = a.view(total_q, hid)
    h = _compose_dev(a2, _unfused(inner, a2), block.mlp.a_pool, block.mlp.b_pool, block.mlp.scaling, ids, cu, max(sq))
    want = inner.down_proj(h)                                                 # the LoRALinear: base + its own shrink / expand
    assert torch.equal(bits(got)[0, live], bits(want)[live]) and torch.isfinite(got[0, live].float()).all()
    pool.clear_batch()
    assert not torch.equal(bits(got)[0, live], bits(block.mlp(a))[0, live])    # no batch: the fused launch and no adapter
    assert torch.equal(bits(block.mlp(a)), bits(inner.down_proj.base(inner.our_llama_mlp(a))))
