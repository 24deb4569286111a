"""not-gpu: multi-LoRA on the gate / up pair on the host -- the oracle (tests/lora_gate_up_oracle.py) against the PEFT composition in float64 on
hand-sized rows, every mutant rejected by the lattice step under the accepted-code hull, the C entry's argument checks (calls that return before any
device call), the refusals of the two ops wrappers, LoRAGateUp's adapter loading on CPU tensors, attach_lora_mlp on a CPU block and the W3 refusal."""
import ctypes

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi, ops
from llm_awq_amd.fused_mlp import QuantLlamaMLP
from llm_awq_amd.lora import LoRAGateUp, LoRALinear, LoRAPool, attach_lora, attach_lora_mlp
from llm_awq_amd.qmodule import WQLinear
from tests import lora_gate_up_oracle as G
from tests import lora_oracle as L
from tests import tail_oracle as TO
from tests.lm_head_oracle import f64, round_T


def test_interleave_is_the_8_plus_8_order_of_the_fused_stream():
    F = 24
    stacked = np.arange(2 * F, dtype=np.float64)[None, :]          # gate row f -> f, up row f -> F + f
    y2 = G.interleave(stacked)[0]
    for f in range(F):
        assert y2[16 * (f // 8) + f % 8] == f and y2[16 * (f // 8) + 8 + f % 8] == F + f
    assert np.array_equal(G.deinterleave(G.interleave(stacked)), stacked)
    t = torch.arange(2 * F, dtype=torch.bfloat16)[None, :]
    assert torch.equal(G.deinterleave(G.interleave(t)), t) and np.array_equal(G.interleave(t).double().numpy()[0], y2)


def _hand_case():
    """K = 4, R = 2, F = 8 (the oracle does not care about the kernel's limits), bf16: sequence 0 (one row) on slot 0, sequence 1 (one row) without
    an adapter, one padding row.  Every value is a small multiple of a power of two, so nothing below rounds except where it says so."""
    T = torch.bfloat16
    K, R, F = 4, 2, 8
    x = torch.tensor([[1, 2, 0, -1], [float("nan")] * 4, [float("nan")] * 4], dtype=T)
    A = torch.zeros(1, 2 * R, K, dtype=T)
    A[0, 0, :2] = torch.tensor([3, 0.5])        # gate: h = (4, 257) -> 0.5 * = (2, 128.5 -> 128, a tie to even)
    A[0, 1, :2] = torch.tensor([1, 128])
    A[0, 2, :2] = torch.tensor([2, 2])          # up:   h = (6, -2) -> (3, -1)
    A[0, 3, :] = torch.tensor([1, -1, 5, 1])
    Bm = torch.zeros(1, 2 * F, R, dtype=T)
    Bm[0, :F, 0] = torch.arange(F) * 0.25 - 1            # B_gate[f] = (f / 4 - 1, 1 / 64)
    Bm[0, :F, 1] = 1 / 64
    Bm[0, F:, 0] = 0.5                                  # B_up[f] = (0.5, f / 8)
    Bm[0, F:, 1] = torch.arange(F) * 0.125
    gate = torch.tensor([[0.5, -1, 2, 0, 1, -3, 4, 0.25]] * 3, dtype=T)
    up = torch.tensor([[1, 2, -1, 0.5, 3, 1, -2, 8]] * 3, dtype=T)
    cu = np.array([0, 1, 2], np.int32)
    ids = np.array([0, -1], np.int32)
    slot = L.row_slots(ids, cu, 2, 3, 1, 1)
    c = dict(K=K, R=R, N=2 * F, slice_end=(F, 2 * F), S=1, B=2, total_q=3, max_sq=1, ldx=K, dtype_name="bf16", x_store=x, a_pool=A, b_pool=Bm,
             scaling=torch.tensor([0.5]), ids=ids, cu=cu, y_init=torch.cat([gate, up], 1), slot=slot, served=np.nonzero(slot >= 0)[0], kplan=(1, K))
    return G._finish(c, F), gate.double().numpy(), up.double().numpy()


def test_oracle_equals_the_peft_composition_in_float64_on_hand_sized_rows():
    c, gate, up = _hand_case()
    F = c["F"]
    assert c["active"].tolist() == [True, True, False] and c["plain"].tolist() == [False, True, False]
    assert torch.isnan(c["y2"][2].float()).all() and np.array_equal(f64(c["y2"])[0, :16], np.concatenate([gate[0], up[0]]))
    g, u, written = G.reference(c)
    assert written.tolist() == [True, True, False]
    # PEFT: W' x = W x + (alpha / r) B (A x), per projection, here with the one rounding of hT the contract takes (128.5 -> 128)
    x0 = np.array([1, 2, 0, -1.0])
    A, Bm = f64(c["a_pool"])[0], f64(c["b_pool"])[0]
    hT = 0.5 * (A @ x0)
    assert hT.tolist() == [2.0, 128.5, 3.0, -1.0]
    hT[1] = 128.0
    g_want, u_want = gate[0] + Bm[:F] @ hT[:2], up[0] + Bm[F:] @ hT[2:]
    assert np.array_equal(g[0], round_T(g_want, "bf16")) and np.array_equal(u[0], round_T(u_want, "bf16"))
    assert np.array_equal(g[0], g_want) and np.array_equal(u[0], u_want)                # (nothing rounds in the sums of this row)
    assert np.array_equal(g[1], gate[1]) and np.array_equal(u[1], up[1])                # no adapter: the pair itself
    lo, hi, _ = G.accepted(c)
    h64 = TO.silu64(np.stack([g_want, gate[1]])) * np.stack([u_want, up[1]])           # silu(g') * u' in float64
    sil = TO.rne64_to_T(TO.silu64(np.stack([g_want, gate[1]])), torch.bfloat16).double().numpy()
    want = G._codes(TO.rne64_to_T(sil * np.stack([u_want, up[1]]), torch.bfloat16))
    assert (((want == lo[:2]) | (want == hi[:2])).all()), "the two-rounding composition in float64 lies outside the accepted codes"
    assert np.allclose(f64(TO.from_bits(np.where(lo[:2] < 0, 0, lo[:2]), torch.bfloat16)), h64, rtol=2.0 ** -6, atol=1e-30)
    assert np.array_equal(lo[2], G._codes(c["h_init"])[2]) and np.array_equal(hi[2], lo[2])       # the padding row keeps its sentinel


@pytest.fixture(scope="module")
def lattice_cases():
    Ku = L.find_uneven_k(L.plan, 32, 2)
    return [G.build_lattice(192, 32, 24, "bf16", **G.PACKED), G.build_lattice(Ku, 32, 24, "fp16", scale_m=3, **G.PACKED),
            G.build_lattice(64, 16, 136, "bf16", max_sq=17, **G.PACKED)]


def test_the_lattice_reference_is_the_lora_oracle_on_the_deinterleaved_pair(lattice_cases):
    for c in lattice_cases:
        F = c["F"]
        g, u, written = G.reference(c)
        exp = f64(c["expected"])                                   # lora_oracle's expected bits on [gate | up]
        rows = c["active"]
        assert np.array_equal(written, rows)
        assert np.array_equal(g[rows], exp[rows, :F]) and np.array_equal(u[rows], exp[rows, F:])
        served = c["slot"] >= 0
        args = L.oracle_args(c)
        d = G._deltas(c, np.nan_to_num(args["a_pool"]), np.nan_to_num(args["b_pool"]))
        assert np.array_equal(round_T(f64(c["y_init"])[served] + d[served], c["dtype_name"]), exp[served])       # _deltas restates steps 1 - 3
        assert c["plain"].sum() == 1 and np.array_equal(g[c["plain"]], f64(c["y_init"])[c["plain"], :F])
        assert torch.isnan(c["y2"][torch.from_numpy(~rows)].float()).all() and torch.isfinite(c["y2"][torch.from_numpy(rows)].float()).all()
        lo, hi, _ = G.accepted(c)
        sent = G._codes(c["h_init"])
        assert np.array_equal(lo[~rows], sent[~rows]) and (lo[rows] != sent[rows]).any() and (lo >= 0).all()
    assert lattice_cases[0]["active"].sum() == 71 and lattice_cases[2]["active"].sum() == 71 - 33                # max_seqlen_q = 17: the 33-row sequence is inactive


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_each_mutant_is_rejected_by_the_lattice_step(mutant, lattice_cases):
    """on at least one element the mutant's two accepted codes are both different from the target's two: no result passes both"""
    for c in lattice_cases[:2]:
        assert G.rejects(c, mutant), f"the packed lattice step (F = {c['F']}, {c['dtype_name']}) does not see the mutant {mutant}"


def test_check_accepts_the_target_and_refuses_a_mutant(lattice_cases):
    c = lattice_cases[0]
    lo, hi, _ = G.accepted(c)
    h = TO.from_bits(np.where(lo < 0, 0x7FC0, lo), torch.bfloat16)
    G.check(c, h)
    m_lo, _, _ = G.accepted(c, "up_delta_dropped")
    with pytest.raises(AssertionError, match="outside the accepted codes"):
        G.check(c, TO.from_bits(np.where(m_lo < 0, 0x7FC0, m_lo), torch.bfloat16))


def test_gpu_shapes_rotate_every_form():
    shapes = G.gpu_shapes()
    assert len(shapes) == 9 and {s[2] for s in shapes} == {8, 24, 136} and {s[1] for s in shapes} == {16, 32, 64}
    for R in (16, 32, 64):
        assert {s[2] for s in shapes if s[1] == R} == {8, 24, 136}
    for K, R, F in shapes:
        p = ops.lora_plan(K, R, 2)
        assert (p["k_splits"], p["k_per_split"]) == L.plan(K, R, 2)
        if K not in (64, 192):
            assert p["k_splits"] >= 2 and (K // 64) % p["k_splits"] != 0


def test_c_abi_refuses_bad_arguments_before_launching():
    lib = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 30

    def f(ws=p, wsb=big, bp=p, sc=p, ids=p, cu=p, y2=p, h=p, b=2, msq=4, tq=8, s=3, n2=16, k=64, r=16, dt=1):
        return lib.awq_lora_expand_gate_up(ws, wsb, bp, sc, ids, cu, y2, h, b, msq, tq, s, n2, k, r, dt, None)

    assert f(ws=None) == -6 and f(bp=None) == -6 and f(sc=None) == -6 and f(ids=None) == -6 and f(y2=None) == -6 and f(h=None) == -6       # null
    assert f(dt=2) == -3                                                                                                              # dtype
    assert f(r=8) == -4 and f(r=48) == -4 and f(k=0) == -4 and f(k=96) == -4                                                          # rank, k
    assert f(n2=0) == -4 and f(n2=8) == -4 and f(n2=24) == -4                                                                         # n2 >= 16, n2 % 16
    assert f(b=0) == -1 and f(b=65536) == -1 and f(msq=0) == -1 and f(msq=1048561) == -1 and f(tq=0) == -1 and f(s=0) == -1           # batch
    assert f(cu=None, b=2, msq=4, tq=9) == -1                                                                                         # rectangular
    assert f(wsb=1 * 8 * 32 * 4 - 1) == -7                                                                                            # KS = 1, total_q = 8, RS = 32
    assert f(ws=p + 8) == -5 and f(bp=p + 8) == -5 and f(y2=p + 2) == -5 and f(h=p + 8) == -5                                         # alignment
    assert f(sc=p + 2) == -5 and f(ids=p + 2) == -5 and f(cu=p + 1) == -5
    # the order of awq_lora_expand: null, dtype, shape, batch, workspace, alignment
    assert f(ws=None, dt=2) == -6 and f(dt=2, r=8) == -3 and f(r=8, b=0) == -4 and f(b=0, wsb=0) == -1 and f(wsb=0, h=p + 8) == -7


def test_ops_refuse_cpu_tensors():
    T = torch.bfloat16
    x, y2 = torch.zeros(4, 64, dtype=T), torch.zeros(4, 32, dtype=T)
    a, b, sc = torch.zeros(3, 32, 64, dtype=T), torch.zeros(3, 32, 16, dtype=T), torch.zeros(3)
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_capi.AwqNativeError, match="y2 must be a GPU tensor"):
        ops.lora_expand_gate_up(torch.zeros(1024), b, sc, ids, y2, 64)
    with pytest.raises(_capi.AwqNativeError, match="x must be a GPU tensor"):
        ops.lora_apply_gate_up(x, y2, a, b, sc, ids)


def test_ops_argument_checks_in_order():
    """the checks behind the device check, reached with tensors that only claim to live on the GPU"""
    T = torch.bfloat16

    class Fake(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    fake = lambda t: t.as_subclass(Fake)
    x, y2 = fake(torch.zeros(4, 64, dtype=T)), fake(torch.zeros(4, 32, dtype=T))
    a, b, sc = fake(torch.zeros(3, 32, 64, dtype=T)), fake(torch.zeros(3, 32, 16, dtype=T)), fake(torch.zeros(3))
    ids, ws = fake(torch.zeros(4, dtype=torch.int32)), fake(torch.zeros(1024))
    E = ops.lora_expand_gate_up
    with pytest.raises(TypeError, match="y2 must be float16 or bfloat16"):
        E(ws, b, sc, ids, fake(torch.zeros(4, 32)), 64)
    with pytest.raises(ValueError, match="y2 must be a"):
        E(ws, b, sc, ids, fake(torch.zeros(32, dtype=T)), 64)
    with pytest.raises(ValueError, match="y2 must be contiguous"):
        E(ws, b, sc, ids, fake(torch.zeros(32, 4, dtype=T).t()), 64)
    with pytest.raises(ValueError, match="a multiple of 16"):
        E(ws, fake(torch.zeros(3, 24, 16, dtype=T)), sc, ids, fake(torch.zeros(4, 24, dtype=T)), 64)
    with pytest.raises(ValueError, match="b_pool must be a contiguous"):
        E(ws, fake(torch.zeros(3, 16, 16, dtype=T)), sc, ids, y2, 64)                       # [S, F, R]: one projection's B only
    with pytest.raises(TypeError, match="b_pool must have the rows' dtype"):
        E(ws, fake(torch.zeros(3, 32, 16, dtype=torch.float16)), sc, ids, y2, 64)
    with pytest.raises(ValueError, match="scaling must be a contiguous float32"):
        E(ws, b, fake(torch.zeros(2)), ids, y2, 64)
    with pytest.raises(TypeError, match="adapter_ids must be int32"):
        E(ws, b, sc, fake(torch.zeros(4, dtype=torch.int64)), y2, 64)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be int32 \[B \+ 1\]"):
        E(ws, b, sc, ids, y2, 64, cu_seqlens_q=fake(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="rectangular"):
        E(ws, b, sc, fake(torch.zeros(3, dtype=torch.int32)), y2, 64)
    with pytest.raises(_capi.AwqNativeError):                                               # the plan refuses k = 96
        E(ws, b, sc, ids, y2, 96)
    with pytest.raises(_capi.AwqNativeError):                                               # ... and rank 8
        E(ws, fake(torch.zeros(3, 32, 8, dtype=T)), sc, ids, y2, 64)
    with pytest.raises(ValueError, match="ws .* is required"):
        E(None, b, sc, ids, y2, 64)
    with pytest.raises(ValueError, match="lora_workspace_bytes asks for"):
        E(fake(torch.zeros(8)), b, sc, ids, y2, 64)
    with pytest.raises(ValueError, match=r"h must be a contiguous \[4, 16\]"):
        E(ws, b, sc, ids, y2, 64, h=fake(torch.zeros(4, 32, dtype=T)))
    with pytest.raises(ValueError, match="h must be a contiguous"):
        E(ws, b, sc, ids, y2, 64, h=fake(torch.zeros(4, 16, dtype=torch.float16)))
    A = ops.lora_apply_gate_up
    with pytest.raises(ValueError, match="same rows"):
        A(x, fake(torch.zeros(5, 32, dtype=T)), a, b, sc, ids)
    with pytest.raises(TypeError, match="y2 must be float16 or bfloat16"):
        A(x, fake(torch.zeros(4, 32)), a, b, sc, ids)
    with pytest.raises(ValueError, match="a_pool must be a contiguous"):                     # a_pool's rows must be 2 R of b_pool
        A(x, y2, fake(torch.zeros(3, 16, 64, dtype=T)), b, sc, ids)
    with pytest.raises(ValueError, match="b_pool must be a contiguous"):
        A(x, y2, a, fake(torch.zeros(3, 48, 16, dtype=T)), sc, ids)


def _cpu_mlp(K=128, F=24, T=torch.bfloat16):
    lin = lambda k, n: WQLinear(4, 128, k, n, False, "cpu", dtype=T)
    return QuantLlamaMLP(lin(K, F), lin(128, K), lin(K, F))


def test_lora_gate_up_load_adapter_and_unload_on_cpu_tensors():
    T = torch.float16
    K, F, R = 128, 24, 16
    pool = LoRAPool(num_slots=2, rank=R, dtype=T, device="cpu")
    gu = LoRAGateUp(_cpu_mlp(K, F, T=T), pool, name="mlp")
    assert tuple(gu.a_pool.shape) == (2, 2 * R, K) and tuple(gu.b_pool.shape) == (2, 2 * F, R) and tuple(gu.scaling.shape) == (2,)
    assert pool.layers == [gu] and gu.lora_name == "mlp" and gu.down_proj is gu.mlp.down_proj
    g = torch.Generator().manual_seed(2)
    Ag, Bg, Au, Bu = torch.randn(5, K, generator=g), torch.randn(F, 5, generator=g), torch.randn(5, K, generator=g), torch.randn(F, 5, generator=g)
    ptrs = (gu.a_pool.data_ptr(), gu.b_pool.data_ptr(), gu.scaling.data_ptr())
    gu.load_adapter(1, {"gate_proj": (Ag, Bg), "up_proj": (Au, Bu)}, alpha=10, rank=5)                  # rank padding: 5 of 16
    assert torch.equal(gu.a_pool[1, :5], Ag.to(T)) and (gu.a_pool[1, 5:R] == 0).all()                    # gate's rows first
    assert torch.equal(gu.a_pool[1, R:R + 5], Au.to(T)) and (gu.a_pool[1, R + 5:] == 0).all()            # then up's
    assert torch.equal(gu.b_pool[1, :F, :5], Bg.to(T)) and torch.equal(gu.b_pool[1, F:, :5], Bu.to(T)) and (gu.b_pool[1, :, 5:] == 0).all()   # natural order
    assert gu.scaling.tolist() == [0.0, 2.0] and (gu.a_pool[0] == 0).all() and (gu.b_pool[0] == 0).all()
    # PEFT keys, a one-sided adapter (up only), in place: gate's half becomes zeros
    gu.load_adapter(1, {"up_proj": {"m.up_proj.lora_A.weight": Au[:3], "m.up_proj.lora_B.weight": Bu[:, :3]}}, alpha=6, rank=3)
    assert ptrs == (gu.a_pool.data_ptr(), gu.b_pool.data_ptr(), gu.scaling.data_ptr())
    assert (gu.a_pool[1, :R] == 0).all() and (gu.b_pool[1, :F] == 0).all()
    assert torch.equal(gu.a_pool[1, R:R + 3], Au[:3].to(T)) and (gu.a_pool[1, R + 3:] == 0).all() and (gu.b_pool[1, F:, 3:] == 0).all()
    assert gu.scaling[1] == 2.0
    gu.load_adapter(0, {"gate_proj": (Ag, Bg)}, alpha=5, rank=5)                                        # gate only
    assert torch.equal(gu.b_pool[0, :F, :5], Bg.to(T)) and (gu.b_pool[0, F:] == 0).all() and (gu.a_pool[0, R:] == 0).all() and gu.scaling[0] == 1.0
    # a refused load writes nothing (the second pair is bad: nothing of the first is written either)
    before = (gu.a_pool.clone(), gu.b_pool.clone(), gu.scaling.clone())
    with pytest.raises(ValueError, match="up_proj expects lora_A.weight"):
        gu.load_adapter(0, {"gate_proj": (Au, Bu), "up_proj": (Au, Bu[:-1])}, alpha=1, rank=5)
    with pytest.raises(ValueError, match="rank 17 outside"):
        gu.load_adapter(0, {"gate_proj": (torch.zeros(17, K), torch.zeros(F, 17))}, alpha=1, rank=17)
    with pytest.raises(ValueError, match="gate_proj and / or up_proj"):
        gu.load_adapter(0, {"down_proj": (Ag, Bg)}, alpha=1, rank=5)
    with pytest.raises(ValueError, match="gate_proj and / or up_proj"):
        gu.load_adapter(0, {}, alpha=1, rank=5)
    with pytest.raises(IndexError):
        gu.load_adapter(2, {"gate_proj": (Ag, Bg)}, alpha=1, rank=5)
    assert all(torch.equal(a, b) for a, b in zip(before, (gu.a_pool, gu.b_pool, gu.scaling)))
    # by layer name through the pool, and unload
    pool.load_adapter(0, {"mlp": {"gate_proj": (Ag, Bg), "up_proj": (Au, Bu)}}, alpha=10, rank=5)
    assert gu.scaling[0] == 2.0 and torch.equal(gu.a_pool[0, R:R + 5], Au.to(T))
    pool.unload(0)
    assert (gu.a_pool[0] == 0).all() and (gu.b_pool[0] == 0).all() and gu.scaling[0] == 0 and gu.scaling[1] == 2.0 and (gu.a_pool[1] != 0).any()
    with pytest.raises(TypeError, match="QuantLlamaMLP is expected"):
        LoRAGateUp(torch.nn.Identity(), pool)


def test_attach_lora_mlp_on_a_cpu_block_and_the_refusals():
    block = torch.nn.Module()
    block.mlp = _cpu_mlp()
    block.other = torch.nn.Linear(4, 4)
    inner, down = block.mlp, block.mlp.down_proj
    pool = LoRAPool(3, 32, torch.bfloat16, "cpu")
    # attach_lora keeps refusing the names of the pair
    for name in ("gate_proj", "up_proj"):
        with pytest.raises(ValueError, match=name):
            attach_lora(block, pool, targets=(name,))
    done = attach_lora_mlp(block, pool)
    assert sorted(done) == ["mlp", "mlp.down_proj"]
    assert isinstance(block.mlp, LoRAGateUp) and block.mlp is done["mlp"] and block.mlp.mlp is inner
    assert isinstance(inner.down_proj, LoRALinear) and inner.down_proj is done["mlp.down_proj"] and inner.down_proj.base is down
    assert tuple(block.mlp.a_pool.shape) == (3, 64, 128) and tuple(block.mlp.b_pool.shape) == (3, 48, 32)
    assert tuple(inner.down_proj.a_pool.shape) == (3, 32, 128) and pool.layers == [done["mlp"], done["mlp.down_proj"]]
    assert [l.lora_name for l in pool.layers] == ["mlp", "mlp.down_proj"]
    with pytest.raises(ValueError, match="no QuantLlamaMLP child"):      # nothing left to attach: the wrapped MLP is not wrapped again
        attach_lora_mlp(block, pool)
    # down_proj=False, and a down_proj that is wrapped already stays as it is
    b2 = torch.nn.Module()
    b2.mlp = _cpu_mlp()
    assert sorted(attach_lora_mlp(b2, LoRAPool(2, 16, torch.bfloat16, "cpu"), down_proj=False)) == ["mlp"] and isinstance(b2.mlp.down_proj, WQLinear)
    b3 = torch.nn.Module()
    b3.mlp = _cpu_mlp()
    p3 = LoRAPool(2, 16, torch.bfloat16, "cpu")
    first = attach_lora(b3, p3, targets=("down_proj",))["mlp.down_proj"]
    assert sorted(attach_lora_mlp(b3, p3)) == ["mlp"] and b3.mlp.down_proj is first
    # W3 is refused by name, and nothing is replaced
    b4 = torch.nn.Module()
    b4.mlp = _cpu_mlp()
    b4.mlp.w_bit = 3
    with pytest.raises(ValueError, match="W3"):
        attach_lora_mlp(b4, p3)
    assert isinstance(b4.mlp, QuantLlamaMLP)
    with pytest.raises(ValueError, match="W3"):
        LoRAGateUp(b4.mlp, p3)
    # with no batch set the wrapper is the module itself (nothing of the adapted path is touched)
    calls = []
    block.mlp.mlp.forward = lambda x: calls.append(x) or x
    x = torch.zeros(2, 128, dtype=torch.bfloat16)
    assert block.mlp(x) is x and len(calls) == 1
