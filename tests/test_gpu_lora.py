"""gpu: multi-LoRA on packed steps (awq_lora_shrink + awq_lora_expand, ops.lora_apply, LoRAPool / LoRALinear / attach_lora) against the float64
oracle of the contract (tests/lora_oracle.py): exact bits on the lattice for decode batches and a packed step, rows outside the contract untouched
(NaN in their x, in the workspace and in unnamed pool slots; a sentinel in their y), independence of the batch and of a loose max_seqlen_q,
determinism, random inputs under the derived bound, one captured graph replayed over changed ids / lengths / adapters, and the modules."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from llm_awq_amd import ops, synth
from llm_awq_amd.lora import LoRALinear, LoRAPool, attach_lora
from tests import lora_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PACKED = dict(sq=O.PACKED_SQ, ids=O.PACKED_IDS, pad=O.PACKED_PAD)
SHAPES = O.gpu_shapes()
shape_id = lambda s: "k%d-r%d-n%d-s%d" % (s[0], s[1], s[2], len(s[3]))


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _run(case, max_sq=None, a_pool=None):
    """ops.lora_apply on a built case: x is the strided view of its storage (ldx = K + 8, NaN in the gap), the workspace is NaN beforehand"""
    K, R, ns = case["K"], case["R"], len(case["slice_end"])
    x = _dev(case["x_store"])[:, :K]
    y = _dev(case["y_init"]).clone()
    ws = torch.full((ops.lora_workspace_bytes(case["total_q"], K, R, ns) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = ops.lora_apply(x, y, _dev(case["a_pool"] if a_pool is None else a_pool), _dev(case["b_pool"]), _dev(case["scaling"]), _dev(case["ids"]),
                         case["slice_end"] if ns > 1 else None, _dev(case["cu"]), case["max_sq"] if max_sq is None else max_sq, ws)
    assert out is y
    return y.cpu()


@functools.lru_cache(maxsize=None)
def _packed_lattice(shape, dtype_name, scale_m=1):
    return O.build_lattice(*shape, dtype_name, scale_m=scale_m, **PACKED)


@pytest.mark.parametrize("B", [1, 2, 17])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lattice_decode_rows_are_exact(shape, dtype_name, B):
    """the rectangular form, one row per sequence: no tolerance, the expected bits are exact (planted ties in h and in y).  With B < 3 some pool
    slot is named by nobody and holds NaN."""
    case = O.build_lattice(*shape, dtype_name, rect=(B, 1))
    assert torch.equal(O.bits(_run(case)), O.bits(case["expected"]))


@pytest.mark.parametrize("scale_m", [1, 3], ids=["pow2", "x1.5"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lattice_packed_step_is_exact_untouched_and_stable(shape, dtype_name, scale_m):
    """Sq = [1, 0, 0, 17, 3, 16, 33, 1] with ids [0, -1, 2, 1, 0, 2, 1, S] and four padding rows: every bit of y, the rows outside the contract
    included (NaN in their x, NaN throughout the workspace, a sentinel in their y).  The same under a max_seqlen_q eight times too loose, and three
    runs give the same bits."""
    case = _packed_lattice(shape, dtype_name, scale_m)
    got = _run(case)
    assert torch.equal(O.bits(got), O.bits(case["expected"]))
    assert torch.equal(O.bits(_run(case, max_sq=8 * case["max_sq"])), O.bits(got))
    assert torch.equal(O.bits(_run(case)), O.bits(got)) and torch.equal(O.bits(_run(case)), O.bits(got))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_an_inactive_sequence_and_a_tight_bound_leave_rows_alone(dtype_name):
    """max_seqlen_q = 17 makes the 33-row sequence inactive: its rows keep their bits, the others their results"""
    shape = SHAPES[4]
    case = O.build_lattice(*shape, dtype_name, max_sq=17, **PACKED)
    assert 37 not in case["served"] and 20 in case["served"]
    assert torch.equal(O.bits(_run(case)), O.bits(case["expected"]))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5], SHAPES[7]], ids=shape_id)
def test_a_rows_bits_do_not_depend_on_its_batch(shape, dtype_name):
    """every sequence of the packed step, run alone through the rectangular call, gives the same bits for its rows"""
    case = _packed_lattice(shape, dtype_name)
    K, ns = case["K"], len(case["slice_end"])
    got = _run(case)
    x, y0 = _dev(case["x_store"])[:, :K], _dev(case["y_init"])
    pools = [_dev(case[n]) for n in ("a_pool", "b_pool", "scaling")]
    seen = 0
    for b, sq in enumerate(O.PACKED_SQ):
        lo = int(case["cu"][b])
        if sq == 0 or not 0 <= case["ids"][b] < case["S"]:
            continue
        y = y0[lo:lo + sq].clone()
        ops.lora_apply(x[lo:lo + sq], y, *pools, _dev(case["ids"][b:b + 1]), case["slice_end"] if ns > 1 else None, None, sq)
        assert torch.equal(O.bits(y), O.bits(got[lo:lo + sq])), b
        seen += 1
    assert seen == 5


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_each_slice_uses_its_own_h_columns(dtype_name):
    """three slices: with the A rows of slice j zeroed the columns of slice j keep y and the other slices keep their results"""
    shape = next(s for s in SHAPES if len(s[3]) == 3 and s[1] == 32)
    case = _packed_lattice(shape, dtype_name)
    R, ends = case["R"], (0,) + case["slice_end"]
    served = torch.from_numpy(case["served"])
    for j in range(3):
        a_pool = case["a_pool"].clone()
        a_pool[:, j * R:(j + 1) * R] = 0
        got = _run(case, a_pool=a_pool)
        want = case["expected"].clone()
        want[served, ends[j]:ends[j + 1]] = case["y_init"][served, ends[j]:ends[j + 1]]
        assert torch.equal(O.bits(got), O.bits(want)), j


RANDOM_SHAPES = [(1024, 64, 80, (48, 64, 80)), (192, 16, 48, (48,)), (O.find_uneven_k(O.plan, 32, 1), 32, 16, (16,)), (4096, 64, 16, (16,))]


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=shape_id)
def test_random_inputs_are_within_the_derived_bound(shape, dtype_name):
    case = O.build_random(*shape, dtype_name, **PACKED)
    ratio = O.check_random(case, _run(case))
    print(f"{shape_id(shape)} {dtype_name}: largest |y - y*| / bound = {ratio:.3f}")
    case = O.build_random(*shape, dtype_name, rect=(5, 1))
    O.check_random(case, _run(case))


class _Base(torch.nn.Module):
    """a stand-in base linear with a fixed output"""

    def __init__(self, y0, k):
        super().__init__()
        self.y0, self.in_features, self.out_features = y0, k, y0.shape[1]

    def forward(self, x):
        return self.y0.clone()


def test_one_graph_replays_changed_ids_lengths_and_adapters():
    """shrink + expand captured once; each replay equals the eager call on the state it finds"""
    K, R, N, ends = 192, 32, 80, (48, 64, 80)
    T = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    cu0, total_q = O.layout(O.PACKED_SQ, O.PACKED_PAD)
    pool = LoRAPool(3, R, T, DEV)
    y0 = torch.randn(total_q, N, generator=g).to(T).to(DEV)
    lin = LoRALinear(_Base(y0, K), pool, slice_end=ends)
    adapter = lambda r: [(torch.randn(r, K, generator=g) / K ** 0.5, 0.05 * torch.randn(w, r, generator=g)) for w in (48, 16, 16)]
    for slot, r in enumerate((32, 8, 16)):
        lin.load_adapter(slot, adapter(r), alpha=2 * r, rank=r)
    x = torch.randn(total_q, K, generator=g).to(T).to(DEV)
    ids, cu = _dev(np.array(O.PACKED_IDS, np.int32)), _dev(cu0)
    pool.set_batch(ids, cu, max(O.PACKED_SQ))
    first = lin(x).clone()          # warm-up: the workspace exists before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lin(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(O.bits(out), O.bits(first)) and not torch.equal(O.bits(first), O.bits(y0))
    seen = [O.bits(first)]

    def step(change):
        change()
        graph.replay()
        got = out.clone()
        want = lin(x)
        torch.cuda.synchronize()
        assert torch.equal(O.bits(got), O.bits(want))
        assert all(not torch.equal(O.bits(got), s) for s in seen), "the change was not seen"
        seen.append(O.bits(got))

    step(lambda: ids.copy_(_dev(np.array([2, 0, 0, 0, -1, 1, 2, 1], np.int32))))
    step(lambda: cu.copy_(_dev(O.layout((4, 16, 0, 1, 33, 0, 2, 15), 0)[0])))
    step(lambda: lin.load_adapter(2, adapter(4), alpha=16, rank=4))
    pool.clear_batch()
    assert torch.equal(O.bits(lin(x)), O.bits(y0))


def _wq(K, N, dtype, seed):
    from llm_awq_amd.qmodule import WQLinear
    c = synth.random_wq(K, N, dtype=dtype, device=DEV, seed=seed, keep_q=False)
    m = WQLinear(4, 128, K, N, False, DEV, dtype=dtype)
    m.load_state_dict(dict(qweight=c["qweight"], scales=c["scales"], scaled_zeros=c["scaled_zeros"]))
    return m


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_lora_linear_over_a_synthetic_wqlinear(dtype_name):
    K, R, N, ends = 256, 16, 80, (48, 64, 80)
    T = O.DTYPES[dtype_name]
    case = O.build_random(K, R, N, ends, dtype_name, **PACKED)
    base = _wq(K, N, T, 3)
    pool = LoRAPool(case["S"], R, T, DEV)
    lin = LoRALinear(base, pool, slice_end=ends)
    with torch.no_grad():
        lin.a_pool.copy_(_dev(case["a_pool"]))
        lin.b_pool.copy_(_dev(case["b_pool"]))
        lin.scaling.copy_(_dev(case["scaling"]))
    x = torch.nan_to_num(_dev(case["x_store"])[:, :K]).contiguous()
    y_base = base(x)
    assert torch.equal(O.bits(lin(x)), O.bits(y_base))                                     # no batch set
    ids, cu = _dev(case["ids"]), _dev(case["cu"])
    pool.set_batch(torch.full_like(ids, -1), cu, case["max_sq"])
    assert torch.equal(O.bits(lin(x)), O.bits(y_base))                                     # nobody has an adapter
    pool.set_batch(ids, cu, case["max_sq"])
    got = lin(x)
    want = ops.lora_apply(x, base(x), lin.a_pool, lin.b_pool, lin.scaling, ids, ends, cu, case["max_sq"])
    assert torch.equal(O.bits(got), O.bits(want)) and not torch.equal(O.bits(got), O.bits(y_base))
    # ... and within the derived bound of the float64 composition on the base output
    case["x_store"] = torch.cat([x.cpu(), case["x_store"][:, K:]], 1)
    case["y_init"] = y_base.cpu()
    case["ideal"], case["bound"] = O.reference(ideal=True, **O.oracle_args(case))
    O.check_random(case, got.cpu())


def test_attach_lora_on_a_packed_attention_step():
    """QuantLlamaAttentionFused(kv_layout="natural").forward_packed with its qkv and o layers adapted: the qkv layer's output inside the step is
    LoRALinear called alone on the same input, and with every id -1 the module returns, on the rows of the step, the bits of the module that was
    never attached"""
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    H, HKV, DH, L = 4, 2, 64, 128
    hid, T = H * DH, torch.bfloat16
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=hid, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    sq = (1, 0, 0, 17, 3, 16, 33, 1)
    B = len(sq)
    make = lambda: QuantLlamaAttentionFused(hid, H, L, _wq(hid, (H + 2 * HKV) * DH, T, 11), _wq(hid, hid, T, 12), DEV, args, max_batch_size=B,
                                            kv_layout="natural")
    plain, adapted = make(), make()
    pool = LoRAPool(3, 16, T, DEV)
    done = attach_lora(adapted, pool)
    assert sorted(done) == ["o_proj", "qkv_proj"] and adapted.qkv_proj.slice_end == (256, 384, 512)
    g = torch.Generator().manual_seed(9)
    for slot in range(3):
        pool.load_adapter(slot, {"qkv_proj": [(torch.randn(8, hid, generator=g) / 16, 0.05 * torch.randn(w, 8, generator=g)) for w in (256, 128, 128)],
                                 "o_proj": (torch.randn(8, hid, generator=g) / 16, 0.05 * torch.randn(hid, 8, generator=g))}, alpha=16, rank=8)
    inv = 1.0 / (10000.0 ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(L, device=DEV).float(), inv)
    freqs = torch.cat([f, f], -1).contiguous()
    cu_np, total_q = O.layout(sq, 4)
    cu, pos = _dev(cu_np), torch.zeros(B, dtype=torch.int32, device=DEV)
    x = (0.5 * torch.randn(1, total_q, hid, generator=g)).to(T).to(DEV)
    step = lambda m: m.forward_packed(x, pos, freqs, cu, max(sq))
    want = step(plain)
    ids = _dev(np.array(O.PACKED_IDS, np.int32))
    pool.set_batch(torch.full_like(ids, -1), cu, max(sq))
    real = int(cu_np[-1])       # the attention leaves the padding rows of its output unwritten: what the module returns there is not defined
    assert torch.equal(O.bits(step(adapted))[0, :real], O.bits(want)[0, :real])
    pool.set_batch(ids, cu, max(sq))
    seen = {}
    hook = adapted.qkv_proj.register_forward_hook(lambda mod, inp, out: seen.update(inp=inp[0].clone(), out=out.clone()))
    got = step(adapted)
    hook.remove()
    alone = adapted.qkv_proj(seen["inp"])
    torch.cuda.synchronize()
    assert torch.equal(O.bits(alone), O.bits(seen["out"]))
    assert not torch.equal(O.bits(seen["out"]), O.bits(plain.qkv_proj(seen["inp"])))
    rows = torch.from_numpy(O.row_slots(np.array(O.PACKED_IDS), cu_np, B, total_q, max(sq), 3) >= 0)
    live = torch.from_numpy(O.owners(cu_np, B, total_q, max(sq)) >= 0)
    assert not torch.equal(O.bits(got)[0, rows], O.bits(want)[0, rows]) and torch.isfinite(got[0, live].float()).all()
