"""not-gpu: the multi-LoRA contract on the host -- the numpy oracle (tests/lora_oracle.py) against hand-worked rows and the PEFT composition, the
derived bound, the invariants of the plan, the mutants, the C ABI's argument checks (calls that return before any device call), the refusals of
ops and LoRAPool / LoRALinear's adapter loading on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi, ops
from llm_awq_amd.lora import LoRALinear, LoRAPool, attach_lora
from tests import lora_oracle as O

PACKED = dict(sq=O.PACKED_SQ, ids=O.PACKED_IDS, pad=O.PACKED_PAD)


def test_oracle_on_hand_worked_rows():
    # K = 4 inside a storage with ldx = 6, one slot, R = 2 (the oracle does not care about the kernel's limits), N = 2, two slices of one column
    K, R, N = 4, 2, 2
    store = np.array([1, 2, 0, 0, 9, 9,          # row 0: sequence 0 (slot 0)
                      1, 1, 0, 0, 9, 9,          # row 1: sequence 1 (no adapter)
                      1, 1, 0, 0, 9, 9], float)  # row 2: padding
    A = np.zeros((1, 2 * R, K))
    A[0, 0, :2] = [3, 0.5]      # slice 0: h = (4, 257)
    A[0, 1, :2] = [1, 128]
    A[0, 2, :2] = [2, 2]        # slice 1: h = (6, -1)
    A[0, 3, :2] = [1, -1]
    Bm = np.zeros((1, N, R))
    Bm[0, 0] = [1.5, 1]
    Bm[0, 1] = [0.25, 4]
    y0 = np.array([[1.0, 0.5], [7.0, 7.0], [5.0, 5.0]])
    kw = dict(ldx=6, total_q=3, a_pool=A, b_pool=Bm, scaling=np.array([0.5], np.float32), ids=[0, -1], cu=[0, 1, 2], max_sq=1, slice_end=(1, 2),
              y_init=y0, dtype_name="bf16", kplan=(1, K))
    y, _ = O.reference(store, **kw)
    # hT = T(0.5 * (4, 257, 6, -1)) = (2, 128.5 -> 128 (tie to even), 3, -0.5); d = (1.5 * 2 + 128, 0.25 * 3 - 2) = (131, -1.25)
    # y = T(1 + 131) = 132, T(0.5 - 1.25) = -0.75; the other rows keep their values
    assert y.tolist() == [[132.0, -0.75], [7.0, 7.0], [5.0, 5.0]]
    ideal, bnd = O.reference(store, ideal=True, **kw)
    assert ideal[0].tolist() == [1 + 1.5 * 2 + 128.5, 0.5 + 0.25 * 3 - 2] and (bnd[1:] == 0).all()
    # mutants by hand
    m = lambda name: O.reference(store, mutant=name, **kw)[0]
    assert m("scaling_dropped")[0].tolist() == [O.round_T(1 + 1.5 * 4 + 256, "bf16"), O.round_T(0.5 + 0.25 * 6 - 4, "bf16")]   # T(257) = 256
    assert m("slice0_h")[0, 1] == O.round_T(0.5 + 0.25 * 2 + 4 * 128, "bf16")
    assert m("no_adapter_slot0")[1].tolist() != [7.0, 7.0] and m("padding_written")[2].tolist() != [5.0, 5.0]
    assert m("h_unrounded")[0, 0] == O.round_T(1 + 3 + 128.5, "bf16") and m("delta_rounded")[0, 1] == O.round_T(0.5 + O.round_T(-1.25, "bf16"), "bf16")
    assert m("ldx_as_k")[0].tolist() == y[0].tolist() and m("ldx_as_k")[1].tolist() == [7.0, 7.0]     # row 0 starts at 0 either way
    assert np.array_equal(O.owners([0, 1, 1, 1, 3], 4, 4, 2), [0, 3, 3, -1]) and np.array_equal(O.owners([0, 1, 1, 1, 3], 4, 4, 2, "owner_first"), [0, -1, -1, -1])
    assert np.array_equal(O.owners([0, 3, 4], 2, 4, 2), [-1, -1, -1, 1])          # Sq_0 = 3 > max_seqlen_q: inactive
    assert np.array_equal(O.owners(None, 2, 4, 2), [0, 0, 1, 1])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_oracle_equals_the_peft_composition_in_float64(dtype_name):
    c = O.build_random(192, 32, 80, (48, 64, 80), dtype_name, **PACKED)
    x = c["x_store"][:, :c["K"]].double()
    want = c["y_init"].double().clone()
    ends = (0,) + c["slice_end"]
    for t in c["served"]:
        a = int(c["slot"][t])
        for j in range(3):
            lo, hi = ends[j], ends[j + 1]
            A = c["a_pool"][a, j * 32:(j + 1) * 32].double()          # lora_A.weight of slice j
            Bm = c["b_pool"][a, lo:hi].double()                       # lora_B.weight of slice j
            want[t, lo:hi] += float(c["scaling"][a]) * torch.nn.functional.linear(torch.nn.functional.linear(x[t], A), Bm)
    got = torch.from_numpy(c["ideal"])
    s = torch.from_numpy(c["served"])
    assert torch.allclose(got[s], want[s], rtol=1e-12, atol=1e-12)
    assert (c["bound"][c["served"]] > 0).all() and (c["bound"][np.setdiff1d(np.arange(c["total_q"]), c["served"])] == 0).all()


def test_the_bound_is_the_derived_one():
    # one row, K = 64, R = 16, N = 16: every term of the docstring's formula written out again
    c = O.build_random(64, 16, 16, (16,), "bf16", rect=(1, 1), ids=[1])
    x = O.f64(c["x_store"])[0, :64]
    A, Bm, y = O.f64(c["a_pool"])[1], O.f64(c["b_pool"])[1], O.f64(c["y_init"])[0]
    sc = float(c["scaling"][1])
    u = 2.0 ** -24
    hs = sc * (A @ x)
    e_h = abs(sc) * 65 * u * (np.abs(A) @ np.abs(x))
    e_h = e_h + O.ulp_T(np.abs(hs) + e_h, "bf16") / 2
    e_d = np.abs(Bm) @ e_h + 17 * u * (np.abs(Bm) @ (np.abs(hs) + e_h) + np.abs(y))
    ystar = y + Bm @ hs
    want = e_d + O.ulp_T(np.abs(ystar) + e_d, "bf16") / 2
    assert np.allclose(c["bound"][0], want, rtol=1e-12) and np.allclose(c["ideal"][0], ystar, rtol=1e-12)
    assert (want >= O.ulp_T(ystar, "bf16") / 2).all() and (want < 4 * O.ulp_T(np.abs(ystar) + 1e-2, "bf16")).all()   # dominated by the last rounding


def test_plan_invariants_for_every_gpu_shape():
    shapes = [(K, R, len(ends)) for K, R, _, ends in O.gpu_shapes(lambda k, r, n: tuple(ops.lora_plan(k, r, n)[f] for f in ("k_splits", "k_per_split")))]
    shapes += [(1024, 64, 3), (192, 16, 1), (O.find_uneven_k(O.plan, 32, 1), 32, 1), (192, 32, 3), (256, 16, 3), (256, 16, 1)]      # random, graph and module tests
    shapes += [(4096, 16, 3), (4096, 64, 3), (4096, 16, 1), (4096, 64, 1), (14336, 16, 1), (14336, 64, 1), (64 * 4097, 64, 3)]
    by_rs = {}
    for K, R, ns in shapes:
        p = ops.lora_plan(K, R, ns)
        ks, kper = p["k_splits"], p["k_per_split"]
        assert (ks, kper) == O.plan(K, R, ns), (K, R, ns)
        assert 1 <= ks <= 32 and kper % 64 == 0 and (ks - 1) * kper < K <= ks * kper, (K, R, ns, p)      # the splits cover K exactly, none is empty
        assert p["col_tile"] % 16 == 0 and p["waves"] == 4
        assert by_rs.setdefault((K, R * ns), (ks, kper)) == (ks, kper)
        for total_q in (1, 17, 75):
            assert ops.lora_workspace_bytes(total_q, K, R, ns) == ks * total_q * R * ns * 4
    # (K, RS) alone: the same RS reached through another (R, n_slices) gives the same split
    for K in (192, 4096, 14336):
        assert ops.lora_plan(K, 32, 1) == ops.lora_plan(K, 16, 2) and ops.lora_plan(K, 64, 1) == ops.lora_plan(K, 32, 2)
    # one decode row over down_proj's K with RS = 64 is not one block's work
    assert ops.lora_plan(14336, 64, 1)["k_splits"] >= 16
    # the uneven K really is uneven
    for K, R, _, ends in O.gpu_shapes():
        ks, kper = O.plan(K, R, len(ends))
        if K not in (64, 192):
            assert ks >= 2 and (K // 64) % ks != 0, (K, R, ends)
    assert ops.lora_workspace_bytes(4, 100, 16, 1) == 0 and ops.lora_workspace_bytes(0, 64, 16, 1) == 0
    with pytest.raises(_capi.AwqNativeError):
        ops.lora_plan(64, 8, 1)


@pytest.fixture(scope="module")
def lattice_cases():
    Ku = O.find_uneven_k(O.plan, 32, 3)
    return [O.build_lattice(192, 32, 80, (48, 64, 80), "bf16", **PACKED),
            O.build_lattice(Ku, 32, 80, (48, 64, 80), "fp16", scale_m=3, **PACKED),
            O.build_lattice(64, 16, 16, (16,), "bf16", rect=(2, 1))]


def test_lattice_cases_hold_ties_and_untouched_rows(lattice_cases):
    for c in lattice_cases:
        K, R, name = c["K"], c["R"], c["dtype_name"]
        xs, Ap, Bp, y0 = O.f64(c["x_store"]), O.f64(c["a_pool"]), O.f64(c["b_pool"]), O.f64(c["y_init"])
        t0, cols = c["h_ties"]
        a = int(c["slot"][t0])
        h = Ap[a] @ xs[t0, :K]
        # scaling * h in lattice units (scaling = m * 2^e: m is folded into the integer) lies half way between two T values, once each way
        assert [O.tie_direction(int(c["scale_m"] * h[col] / c["h_unit"]), name) for col in cols] == ["up", "down"]
        for want, (t, n) in c["y_ties"].items():
            a, j = int(c["slot"][t]), O.slice_of(n, c["slice_end"])
            hs = (np.float32(c["scaling"][a]) * (Ap[a, j * R:(j + 1) * R] @ xs[t, :K]).astype(np.float32)).astype(np.float64)
            s = y0[t, n] + Bp[a, n] @ O.round_T(hs, name)                # exact in float64: every term is a small integer of lattice units
            assert s / c["d_unit"][t] == np.rint(s / c["d_unit"][t]) and O.tie_direction(int(s / c["d_unit"][t]), name) == want
            assert O.f64(c["expected"])[t, n] == O.round_T(s, name) != s
        rest =np.setdiff1d(np.arange(c["total_q"]), c["served"])
        assert torch.equal(O.bits(c["expected"])[rest], O.bits(c["y_init"])[rest])
        assert not torch.equal(O.bits(c["expected"])[c["served"]], O.bits(c["y_init"])[c["served"]])
        assert torch.isnan(c["x_store"][rest].float()).all() and torch.isnan(c["x_store"][:, c["K"]:].float()).all()
    assert sorted(lattice_cases[0]["served"].tolist()) == [0] + list(range(1, 18)) + list(range(18, 21)) + list(range(21, 37)) + list(range(37, 70))
    assert torch.isnan(lattice_cases[2]["a_pool"][2].float()).all()      # a slot nobody names is poisoned


@pytest.mark.parametrize("mutant", O.MUTANTS)
def test_each_mutant_is_rejected_by_a_built_case(mutant, lattice_cases):
    hit = False
    for c in lattice_cases:
        if not torch.equal(O.bits(O.expected_bits(c, mutant)), O.bits(c["expected"])):      # bound zero: any other bit is a rejection
            hit = True
    assert hit, f"no lattice case sees the mutant {mutant}"
    if mutant in O.ROUNDING_MUTANTS:
        return
    beyond = False
    for c in (O.build_random(192, 32, 80, (48, 64, 80), "bf16", **PACKED), O.build_random(O.find_uneven_k(O.plan, 32, 3), 32, 80, (48, 64, 80), "fp16", **PACKED)):
        y, _ = O.reference(ideal=True, mutant=mutant, **O.oracle_args(c))
        rows = np.arange(c["total_q"])
        with np.errstate(invalid="ignore"):
            err = np.abs(O.round_T(np.nan_to_num(y), c["dtype_name"]) - np.where(c["bound"] > 0, c["ideal"], O.f64(c["y_init"])))
            bad = ~np.isfinite(y) | (err > c["bound"])
        beyond |= bool(bad[rows].any())
    assert beyond, f"no random case puts the mutant {mutant} beyond the derived bound"


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 30
    ends = (ctypes.c_int * 3)(48, 64, 80)
    one = (ctypes.c_int * 1)(16)

    def shrink(x=p, ldx=64, a=p, ids=p, cu=p, ws=p, wsb=big, b=2, msq=4, tq=8, s=3, k=64, r=16, ns=1, dt=1):
        return L.awq_lora_shrink(x, ldx, a, ids, cu, ws, wsb, b, msq, tq, s, k, r, ns, dt, None)

    def expand(ws=p, wsb=big, bp=p, sc=p, ids=p, cu=p, y=p, b=2, msq=4, tq=8, s=3, n=16, k=64, r=16, se=one, ns=1, dt=1):
        return L.awq_lora_expand(ws, wsb, bp, sc, ids, cu, y, b, msq, tq, s, n, k, r, se, ns, dt, None)

    for f in (shrink, expand):
        assert f(dt=2) == -3                                                             # dtype
        assert f(r=8) == -4 and f(r=48) == -4 and f(ns=0) == -4 and f(ns=4) == -4        # rank, slices
        assert f(k=0) == -4 and f(k=96) == -4                                            # k >= 64, k % 64
        assert f(b=0) == -1 and f(b=65536) == -1 and f(msq=0) == -1 and f(tq=0) == -1 and f(s=0) == -1
        assert f(cu=None, b=2, msq=4, tq=9) == -1                                        # rectangular: total_q = B * max_seqlen_q
        assert f(wsb=1 * 8 * 16 * 4 - 1) == -7                                           # KS = 1, total_q = 8, RS = 16
        assert f(ids=None) == -6 and f(ws=None) == -6
        assert f(ids=p + 2) == -5 and f(cu=p + 1) == -5 and f(ws=p + 8) == -5
    assert shrink(ldx=63) == -4 and shrink(ldx=68) == -4 and shrink(x=None) == -6 and shrink(a=None) == -6
    assert shrink(x=p + 8) == -5 and shrink(a=p + 4) == -5
    assert expand(n=24, se=(ctypes.c_int * 1)(24)) == -4                                 # n % 16
    assert expand(n=80, se=ends, ns=3, wsb=8 * 48 * 4 - 1) == -7                         # a valid slice list passes the shape checks (RS = 48)
    for bad in ((48, 48, 80), (48, 40, 80), (48, 64, 96), (48, 60, 80), (0, 64, 80)):
        assert expand(n=80, se=(ctypes.c_int * 3)(*bad), ns=3) == -4, bad
    assert expand(n=80, se=(ctypes.c_int * 2)(48, 64), ns=2) == -4                        # the last end is not n
    assert expand(bp=None) == -6 and expand(sc=None) == -6 and expand(y=None) == -6 and expand(se=None) == -6
    assert expand(bp=p + 8) == -5 and expand(y=p + 2) == -5 and expand(sc=p + 2) == -5
    out = (ctypes.c_int * 4)()
    assert L.awq_lora_plan(64, 16, 1, None) == -6 and L.awq_lora_plan(32, 16, 1, out) == -4 and L.awq_lora_plan(64, 16, 1, out) == 0
    assert L.awq_lora_workspace_bytes(8, 64, 16, 1) == 8 * 16 * 4


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    T = torch.bfloat16
    x, y = torch.zeros(4, 64, dtype=T), torch.zeros(4, 16, dtype=T)
    a, b, sc = torch.zeros(3, 16, 64, dtype=T), torch.zeros(3, 16, 16, dtype=T), torch.zeros(3)
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_capi.AwqNativeError, match="x must be a GPU tensor"):
        ops.lora_apply(x, y, a, b, sc, ids)
    with pytest.raises(_capi.AwqNativeError, match="x must be a GPU tensor"):
        ops.lora_shrink(x, a, ids, 16)
    with pytest.raises(_capi.AwqNativeError, match="y must be a GPU tensor"):
        ops.lora_expand(torch.zeros(256), b, sc, ids, y, 64)
    with pytest.raises(_capi.AwqNativeError, match="GPU"):
        LoRALinear(torch.nn.Identity(), _cpu_pool_with_batch(), in_features=64, out_features=16)(x)


def _cpu_pool_with_batch():
    pool = LoRAPool(2, 16, torch.bfloat16, "cpu")
    pool.set_batch(torch.zeros(4, dtype=torch.int32))
    return pool


def test_ops_argument_checks_in_order():
    """the checks behind the device check, reached with tensors that only claim to live on the GPU"""
    T = torch.bfloat16

    class Fake(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    fake = lambda t: t.as_subclass(Fake)
    x, y = fake(torch.zeros(4, 64, dtype=T)), fake(torch.zeros(4, 16, dtype=T))
    a, b, sc = fake(torch.zeros(3, 16, 64, dtype=T)), fake(torch.zeros(3, 16, 16, dtype=T)), fake(torch.zeros(3))
    ids = fake(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="x must be float16 or bfloat16"):
        ops.lora_shrink(fake(torch.zeros(4, 64)), a, ids, 16)
    with pytest.raises(ValueError, match="x must be a"):
        ops.lora_shrink(fake(torch.zeros(64, dtype=T)), a, ids, 16)
    with pytest.raises(TypeError, match="adapter_ids must be int32"):
        ops.lora_shrink(x, a, fake(torch.zeros(4, dtype=torch.int64)), 16)
    with pytest.raises(TypeError, match="cu_seqlens_q must be int32"):
        ops.lora_shrink(x, a, ids, 16, cu_seqlens_q=fake(torch.zeros(5, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be int32 \[B \+ 1\]"):
        ops.lora_shrink(x, a, ids, 16, cu_seqlens_q=fake(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="a_pool must be a contiguous"):
        ops.lora_shrink(x, fake(torch.zeros(3, 64, 16, dtype=T).transpose(1, 2)), ids, 16)
    with pytest.raises(ValueError, match="a_pool must be a contiguous"):
        ops.lora_shrink(x, fake(torch.zeros(3, 16, 128, dtype=T)), ids, 16)
    with pytest.raises(TypeError, match="a_pool must have the rows' dtype"):
        ops.lora_shrink(x, fake(torch.zeros(3, 16, 64, dtype=torch.float16)), ids, 16)
    with pytest.raises(ValueError, match="not a multiple of rank"):
        ops.lora_shrink(x, a, ids, 32)
    with pytest.raises(ValueError, match="rectangular"):
        ops.lora_shrink(x, a, fake(torch.zeros(3, dtype=torch.int32)), 16)
    with pytest.raises(_capi.AwqNativeError):                                    # the plan refuses rank 8 before anything is allocated
        ops.lora_shrink(x, fake(torch.zeros(3, 8, 64, dtype=T)), ids, 8)
    with pytest.raises(ValueError, match="b_pool must be a contiguous"):
        ops.lora_expand(fake(torch.zeros(256)), fake(torch.zeros(3, 32, 16, dtype=T)), sc, ids, y, 64)
    with pytest.raises(ValueError, match="scaling must be a contiguous float32"):
        ops.lora_expand(fake(torch.zeros(256)), b, fake(torch.zeros(3, dtype=T)), ids, y, 64)
    with pytest.raises(ValueError, match="slice_end must hold"):
        ops.lora_expand(fake(torch.zeros(256)), b, sc, ids, y, 64, slice_end=(4, 8, 12, 16))
    with pytest.raises(ValueError, match="lora_workspace_bytes asks for"):
        ops.lora_expand(fake(torch.zeros(8)), b, sc, ids, y, 64)
    with pytest.raises(ValueError, match="same rows"):
        ops.lora_apply(x, fake(torch.zeros(5, 16, dtype=T)), a, b, sc, ids)
    with pytest.raises(ValueError, match="a_pool must be a contiguous"):          # a_pool's RS must be n_slices * R of b_pool
        ops.lora_apply(x, y, fake(torch.zeros(3, 32, 64, dtype=T)), b, sc, ids)


def test_lora_pool_and_load_adapter_on_cpu_tensors():
    T = torch.float16
    pool = LoRAPool(num_slots=2, rank=16, dtype=T, device="cpu")
    K, N = 64, 48
    lin = LoRALinear(torch.nn.Identity(), pool, in_features=K, out_features=N, name="o_proj")
    g = torch.Generator().manual_seed(1)
    A, Bm = torch.randn(5, K, generator=g), torch.randn(N, 5, generator=g)
    lin.load_adapter(1, (A, Bm), alpha=10, rank=5)
    assert torch.equal(lin.a_pool[1, :5], A.to(T)) and (lin.a_pool[1, 5:] == 0).all() and (lin.a_pool[0] == 0).all()
    assert torch.equal(lin.b_pool[1, :, :5], Bm.to(T)) and (lin.b_pool[1, :, 5:] == 0).all()
    assert lin.scaling.tolist() == [0.0, 2.0]
    ptrs = (lin.a_pool.data_ptr(), lin.b_pool.data_ptr(), lin.scaling.data_ptr())
    lin.load_adapter(1, {"base_model.o_proj.lora_A.weight": A[:3], "base_model.o_proj.lora_B.weight": Bm[:, :3]}, alpha=6, rank=3)     # PEFT keys; in place
    assert ptrs == (lin.a_pool.data_ptr(), lin.b_pool.data_ptr(), lin.scaling.data_ptr())
    assert (lin.a_pool[1, 3:] == 0).all() and (lin.b_pool[1, :, 3:] == 0).all() and lin.scaling[1] == 2.0 and torch.equal(lin.a_pool[1, :3], A[:3].to(T))
    with pytest.raises(ValueError, match="rank 17 outside"):
        lin.load_adapter(0, (torch.zeros(17, K), torch.zeros(N, 17)), alpha=1, rank=17)
    with pytest.raises(ValueError, match="expects lora_A.weight"):
        lin.load_adapter(0, (torch.zeros(4, K + 1), torch.zeros(N, 4)), alpha=1, rank=4)
    with pytest.raises(IndexError):
        lin.load_adapter(2, (A, Bm), alpha=1, rank=5)
    assert (lin.a_pool[0] == 0).all() and lin.scaling[0] == 0          # a refused load wrote nothing
    # a sliced layer: one pair per slice, rows j R .. of A and the slice's columns of B
    qkv = LoRALinear(torch.nn.Identity(), pool, slice_end=(32, 48, 64), in_features=K, out_features=64, name="qkv_proj")
    pairs = {n: (torch.randn(4, K, generator=g), torch.randn(w, 4, generator=g)) for n, w in (("q", 32), ("k", 16), ("v", 16))}
    qkv.load_adapter(0, pairs, alpha=8, rank=4)
    for j, (n, lo, hi) in enumerate((("q", 0, 32), ("k", 32, 48), ("v", 48, 64))):
        assert torch.equal(qkv.a_pool[0, 16 * j:16 * j + 4], pairs[n][0].to(T)) and (qkv.a_pool[0, 16 * j + 4:16 * j + 16] == 0).all()
        assert torch.equal(qkv.b_pool[0, lo:hi, :4], pairs[n][1].to(T)) and (qkv.b_pool[0, lo:hi, 4:] == 0).all()
    assert qkv.scaling[0] == 2.0
    with pytest.raises(ValueError, match="2 .A, B. pairs for 3 slices"):
        qkv.load_adapter(0, [pairs["q"], pairs["k"]], alpha=8, rank=4)
    # by layer name through the pool, and unload
    pool.load_adapter(0, {"o_proj": (A, Bm)}, alpha=5, rank=5)
    assert lin.scaling[0] == 1.0 and torch.equal(lin.a_pool[0, :5], A.to(T))
    with pytest.raises(KeyError):
        pool.load_adapter(0, {"down_proj": (A, Bm)}, alpha=5, rank=5)
    pool.unload(0)
    assert (lin.a_pool[0] == 0).all() and (lin.b_pool[0] == 0).all() and lin.scaling[0] == 0 and (qkv.b_pool[0] == 0).all() and lin.scaling[1] == 2.0
    # batch state: references, not copies; no batch = the base output itself
    ids, cu = torch.tensor([0, -1], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int32)
    pool.set_batch(ids, cu, 2)
    assert pool.adapter_ids is ids and pool.cu_seqlens_q is cu and pool.max_seqlen_q == 2 and pool.has_batch
    pool.clear_batch()
    assert not pool.has_batch
    x = torch.randn(3, K).to(T)
    assert lin(x) is not None and torch.equal(lin(x), x)
    for bad in (dict(adapter_ids=ids.long()), dict(adapter_ids=ids, cu_seqlens_q=cu[:2]), dict(adapter_ids=ids, max_seqlen_q=0)):
        with pytest.raises(ValueError):
            pool.set_batch(**bad)
    with pytest.raises(ValueError, match="rank 8 is not supported"):
        LoRAPool(2, 8)
    with pytest.raises(ValueError, match="slice_end"):
        LoRALinear(torch.nn.Identity(), pool, slice_end=(32, 40, 64), in_features=K, out_features=64)


def test_attach_lora_wraps_the_named_wqlinears_and_refuses_gate_up():
    from types import SimpleNamespace
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    from llm_awq_amd.qmodule import WQLinear
    H, HKV, DH = 4, 2, 64
    hid = H * DH
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=hid, rope_theta=10000.0, rope_scaling=None, max_position_embeddings=64)
    qkv = WQLinear(4, 128, hid, (H + 2 * HKV) * DH, False, "cpu", dtype=torch.bfloat16)
    o = WQLinear(4, 128, hid, hid, False, "cpu", dtype=torch.bfloat16)
    attn = QuantLlamaAttentionFused(hid, H, 64, qkv, o, "cpu", args, max_batch_size=1, kv_layout="natural")
    block = torch.nn.Module()
    block.self_attn = attn
    block.mlp = torch.nn.Module()
    block.mlp.down_proj = WQLinear(4, 128, 512, hid, False, "cpu", dtype=torch.bfloat16)
    block.mlp.other = torch.nn.Linear(4, 4)
    pool = LoRAPool(3, 32, torch.bfloat16, "cpu")
    done = attach_lora(block, pool)
    assert sorted(done) == ["mlp.down_proj", "self_attn.o_proj", "self_attn.qkv_proj"]
    assert attn.qkv_proj.slice_end == (256, 384, 512) and attn.qkv_proj.base is qkv and attn.o_proj.slice_end == (hid,) and attn.o_proj.base is o
    assert tuple(attn.qkv_proj.a_pool.shape) == (3, 96, hid) and tuple(block.mlp.down_proj.a_pool.shape) == (3, 32, 512)
    assert pool.layers == [done[n] for n in ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.down_proj")]
    assert block.mlp.down_proj.layout == "v2" and block.mlp.down_proj.in_features == 512      # what QuantLlamaMLP reads of its down_proj
    with pytest.raises(ValueError, match="gate_proj"):
        attach_lora(block, pool, targets=("gate_proj",))
    with pytest.raises(ValueError, match="no WQLinear child"):
        attach_lora(torch.nn.Linear(4, 4), pool)
