"""not-gpu: the LM-head contract on the host -- the numpy oracle (tests/lm_head_oracle.py) against hand-worked rows, the invariants of the lattice
builders and of the launch plan for every shape the GPU tests use, the proof that each check of the GPU tests sees its fault (one oracle mutant per
fault, each rejected by at least one built case), and the argument checks of both C entries, which need no launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi, ops
from tests import lm_head_oracle as O


def test_oracle_on_hand_worked_rows():
    # two rows of x inside a storage with ldx = 16, K = 8; W has three rows
    store = np.zeros(32)
    store[0:8] = [1, 2, 3, 4, 0, 0, 0, 0.5]
    store[16:24] = [-1, 0, 0, 0, 0, 0, 0, 2]
    w = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 4], [2, 0, 0, -1, 0, 0, 0, 0]], dtype=np.float64)
    bias = np.array([0.5, -1.0, 0.0])
    y, absdot = O.reference(store, 16, 2, w, bias)
    assert y.tolist() == [[10.5, 1.0, -2.0], [-0.5, 7.0, -2.0]]
    assert absdot.tolist() == [[10.5, 3.0, 6.0], [1.5, 9.0, 2.0]]
    # step 0: an inactive row keeps what the output held
    y, _ = O.reference(store, 16, 2, w, bias, seqlens=[4, -1], out_init=np.full((2, 3), 9.0))
    assert y.tolist() == [[10.5, 1.0, -2.0], [9.0, 9.0, 9.0]]
    # step 3: one rounding to T, ties to even -- bf16 holds 8 significant bits, fp16 11
    assert O.round_T([257.0, 259.0, 258.0, -257.0, 0.0, 1.0 + 2.0 ** -9], "bf16").tolist() == [256.0, 260.0, 258.0, -256.0, 0.0, 1.0]
    assert O.round_T([2049.0, 2051.0, 2050.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], "fp16").tolist() == [2048.0, 2052.0, 2050.0, 1.0, 1.0 + 2.0 ** -9]
    assert O.round_T([259.0, -259.0], "bf16", truncate=True).tolist() == [258.0, -258.0]
    for name, T in O.DTYPES.items():     # the same rounding torch does from fp32
        v = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 37
        assert np.array_equal(O.round_T(v.double().numpy(), name), v.to(T).double().numpy())
    # step 1: x = (3, 4, 0 ...), K = 8: mean square 25 / 8, rstd = 0.5657; gamma 2 on the first column
    x = np.array([[3.0, 4, 0, 0, 0, 0, 0, 0]])
    gamma = np.array([2.0, 1, 1, 1, 1, 1, 1, 1])
    xn = O.norm(x, gamma, 0.0, "bf16")
    rstd = 1 / np.sqrt(25 / 8)
    assert xn[0, 2:].tolist() == [0.0] * 6 and xn[0, 0] == O.round_T(6 * rstd, "bf16") and xn[0, 1] == O.round_T(4 * rstd, "bf16")
    assert O.norm(x, gamma, 25 / 8 * 3, "bf16")[0, 1] == O.round_T(4 * rstd / 2, "bf16")   # eps inside the root: mean + eps = 4 mean
    # the embedding: zeros for every id outside the table
    table = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert O.embed_reference([2, -1, 4, 0, 2 ** 31 - 1], table).tolist() == [[6, 7, 8], [0, 0, 0], [0, 0, 0], [0, 1, 2], [0, 0, 0]]


def test_the_bound_is_the_derived_one():
    absdot = np.array([[100.0]])
    assert O.bound(absdot, 4096)[0, 0] == 4097 * 2.0 ** -24 * 100.0
    b = O.bound(absdot, 4096, out="T", dtype_name="bf16", y=np.array([[3.0]]))[0, 0]
    assert b == 4097 * 2.0 ** -24 * 100.0 + 2.0 ** -6 / 2     # ulp of bf16 in [2, 4) is 2^-6


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_lattice_cases_are_exact_in_fp32_and_hold_ties(dtype_name):
    assert max(K for _, _, K in O.LATTICE_SHAPES) * O.R * O.R + O.R < 2 ** 24
    assert {K for _, _, K in O.LATTICE_SHAPES} == {8, 40, 72, 136, 1032} and {V for _, V, _ in O.LATTICE_SHAPES} == {1, 15, 16, 17, 127, 1025}
    assert {M for M, _, _ in O.LATTICE_SHAPES} == {1, 2, 7, 15, 16, 17, 33, 64}
    tie_cases = 0
    for (M, V, K) in O.LATTICE_SHAPES:
        if M * V * K > 2_000_000:
            continue  # (built and asserted by the GPU test; the builder's own assertions are the same)
        for with_bias in (False, True):
            c = O.build_lattice(M, V, K, dtype_name, with_bias)
            y = c["y_f32"]
            assert np.array_equal(y.astype(np.float32).astype(np.float64), y)                      # representable: equality is a fair demand
            assert np.array_equal(O.round_T(c["y_T"], dtype_name), c["y_T"])
            assert torch.isnan(c["x3"][:, :2, :]).all() and not torch.isnan(c["x3"][:, 2, :]).any()
            if c["ties"]:
                tie_cases += 1
                u = O.ulp_T(y[0, c["ties"]], dtype_name)
                assert (np.abs(y[0, c["ties"]] / u) % 1.0 == 0.5).all()                              # exactly half way between two T values
                assert (c["y_T"][0, c["ties"]] / u % 2 == 0).all()                                   # ... and rounded to the even one
    assert tie_cases >= 10
    for (M, V, K) in O.NORM_SHAPES:
        for eps in O.EPS:
            c = O.build_norm_lattice(M, V, K, dtype_name, eps)
            ss = (O.f64(c["x"]) ** 2).sum(-1)
            assert K * O.R * O.R < 2 ** 24 and np.array_equal(ss.astype(np.float32).astype(np.float64), ss)
            if eps:
                assert eps / 8 < ss[0] / K < eps * 8                                                # eps decides row 0's rstd


def test_plan_invariants_for_every_gpu_shape():
    shapes = O.LATTICE_SHAPES + O.RANDOM_SHAPES + O.NORM_SHAPES + [(1, 128256, 4096), (8, 128256, 4096), (64, 32000, 4096), (4, 1025, 136)]
    shapes.append((2, O.planned_v(ops.lm_head_plan), 64))
    for (M, V, K) in shapes:
        p = ops.lm_head_plan(M, V, K)
        tiles = -(-V // p["tile_rows"])
        assert p["tile_rows"] == O.reference.__defaults__[-1] and p["tile_rows"] % 16 == 0 and p["waves"] == p["k_split"] == 4
        assert 1 <= p["blocks"] <= min(tiles, 512)
        rounds = -(-tiles // p["blocks"])
        assert rounds == -(-tiles // 512)                    # no more rounds than the fullest grid needs
        assert p == ops.lm_head_plan(1, V, K)                # the grid does not depend on the row count
    V = O.planned_v(ops.lm_head_plan)
    p = ops.lm_head_plan(2, V, 64)
    assert -(-V // p["tile_rows"]) > p["blocks"] and V % p["tile_rows"] != 0
    for bad in ((0, 10, 8), (65, 10, 8), (1, 0, 8), (1, 10, 4), (1, 10, 12)):
        with pytest.raises(_capi.AwqNativeError):
            ops.lm_head_plan(*bad)


def _rejected_lattice(case, out, mutant, **kw):
    w, bias = O.f64(case["w"]), None if case["bias"] is None else O.f64(case["bias"])
    a = O.reference(case["x_store"], case["ldx"], case["M"], w, bias, out=out, dtype_name=case["dtype_name"], **kw)[0]
    b = O.reference(case["x_store"], case["ldx"], case["M"], w, bias, out=out, dtype_name=case["dtype_name"], mutant=mutant, **kw)[0]
    return not np.array_equal(a, b, equal_nan=True)       # the lattice tests demand equality: any difference is seen


def _rejected_norm(case, mutant):
    x, g, w = O.f64(case["x"]), O.f64(case["gamma"]), O.f64(case["w"])
    a, absdot = O.reference(x, case["K"], case["M"], w, gamma=g, eps=case["eps"], dtype_name=case["dtype_name"])
    b, _ = O.reference(x, case["K"], case["M"], w, gamma=g, eps=case["eps"], dtype_name=case["dtype_name"], mutant=mutant)
    return bool((np.abs(a - b) > O.bound(absdot, case["K"])).any())   # beyond the bound of the random-input test


@pytest.mark.parametrize("mutant", O.MUTANTS)
def test_each_mutant_is_rejected_by_a_built_case(mutant):
    plain = O.build_lattice(2, 15, 40, "bf16", False)
    biased = O.build_lattice(7, 16, 72, "fp16", True)
    normed = O.build_norm_lattice(5, 130, 72, "bf16", 1e-2)
    M = 33
    seq = O.inactive_patterns(M)[1]
    nan_case = O.build_lattice(M, 16, 1032, "bf16", False)
    store = nan_case["x_store"].copy()
    store[(M // 2) * nan_case["ldx"]: (M // 2) * nan_case["ldx"] + nan_case["K"]] = np.nan     # the inactive row holds NaN
    nan_case = dict(nan_case, x_store=store)
    sentinel = np.full((M, 16), -7.0)
    hits = {
        "k_tail": lambda: _rejected_lattice(plain, "f32", mutant),
        "v_tail": lambda: _rejected_lattice(plain, "f32", mutant),
        "row_prev": lambda: _rejected_lattice(plain, "f32", mutant),
        "ldx_as_k": lambda: _rejected_lattice(plain, "f32", mutant),
        "no_gamma": lambda: _rejected_norm(normed, mutant),
        "eps_outside": lambda: _rejected_norm(normed, mutant),
        "xn_unrounded": lambda: _rejected_norm(normed, mutant),
        "bias_per_split": lambda: _rejected_lattice(biased, "f32", mutant),
        "bias_T_first": lambda: _rejected_lattice(biased, "f32", mutant),
        "trunc": lambda: _rejected_lattice(biased, "T", mutant) and _rejected_lattice(plain, "T", mutant),
        "inactive_written": lambda: _rejected_lattice(nan_case, "f32", mutant, seqlens=seq, out_init=sentinel),
        "nan_leak": lambda: _rejected_lattice(nan_case, "f32", mutant, seqlens=seq, out_init=sentinel),
    }
    assert set(hits) == set(O.MUTANTS)
    assert hits[mutant](), mutant
    # and the unmutated oracle agrees with itself on the same case (the check is not one that rejects everything)
    assert not _rejected_lattice(plain, "f32", None) and not _rejected_norm(normed, None)


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    BATCH, DTYPE, SHAPE, ALIGN, NULL = -1, -3, -4, -5, -6
    names = ("x", "gamma", "weight", "bias", "seqlens", "out")

    def call(m=4, v=100, k=64, ldx=64, dt=1, odt=2, mb=0, eps=1e-6, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        return L.awq_lm_head(a["x"], ldx, a["gamma"], eps, a["weight"], a["bias"], a["seqlens"], a["out"], odt, m, v, k, dt, mb, None)

    for n in ("x", "weight", "out"):
        assert call(**{n: None}) == NULL, n
    assert call(dt=2) == DTYPE and call(dt=-1) == DTYPE and call(dt=3) == DTYPE
    assert call(dt=1, odt=0) == DTYPE and call(dt=0, odt=1) == DTYPE and call(odt=3) == DTYPE      # the output is fp32 or x's own dtype
    assert call(m=0) == BATCH and call(m=65) == BATCH and call(m=-1) == BATCH
    assert call(v=0) == SHAPE and call(k=0) == SHAPE and call(k=4) == SHAPE and call(k=68, ldx=72) == SHAPE
    assert call(ldx=56) == SHAPE and call(ldx=68) == SHAPE and call(ldx=0) == SHAPE and call(mb=-1) == SHAPE
    for n in ("x", "weight", "out", "gamma", "bias"):
        assert call(**{n: p + 8}) == ALIGN, n
    assert call(seqlens=p + 2) == ALIGN
    plan = (ctypes.c_int * 4)()
    assert L.awq_lm_head_plan(1, 10, 8, None) == NULL and L.awq_lm_head_plan(65, 10, 8, plan) == BATCH and L.awq_lm_head_plan(1, 10, 9, plan) == SHAPE
    assert L.awq_lm_head_plan(64, 1, 8, plan) == 0 and list(plan) == [1, 64, 4, 4]

    def emb(n=3, v=10, k=64, dt=1, tokens=p, table=p, out=p):
        return L.awq_embed_tokens(tokens, table, out, n, v, k, dt, None)

    assert emb(tokens=None) == NULL and emb(table=None) == NULL and emb(out=None) == NULL
    assert emb(dt=2) == DTYPE and emb(n=0) == SHAPE and emb(v=0) == SHAPE and emb(k=0) == SHAPE and emb(k=12) == SHAPE
    assert emb(table=p + 8) == ALIGN and emb(out=p + 4) == ALIGN and emb(tokens=p + 2) == ALIGN
    assert L.awq_abi_version() == 1


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    x, w = torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(8, 16, dtype=torch.bfloat16)
    with pytest.raises(_capi.AwqNativeError):
        ops.lm_head(x, w)
    with pytest.raises(_capi.AwqNativeError):
        ops.embed_tokens(torch.zeros(2, dtype=torch.int32), w)
    with pytest.raises(ValueError):
        ops.lm_head(x.view(-1), w)
    assert list(inspect.signature(ops.lm_head).parameters) == ["x", "weight", "gamma", "eps", "bias", "seqlens", "out", "out_dtype", "max_blocks"]
    assert list(inspect.signature(ops.embed_tokens).parameters) == ["tokens", "table"]
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    for name in ("lm_head", "embed_tokens"):
        doc = getattr(eng, name).__doc__.splitlines()[0]
        assert [s.split(":")[0].strip() for s in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")] == list(
            inspect.signature(getattr(ops, name)).parameters)
    from llm_awq_amd.lm_head import LMHead, TokenEmbedding
    lin = torch.nn.Linear(16, 8, bias=False, dtype=torch.bfloat16)
    norm = torch.nn.Module()
    norm.weight, norm.variance_epsilon = torch.nn.Parameter(torch.ones(16, dtype=torch.bfloat16)), 1e-5
    head = LMHead.from_modules(norm, lin)
    assert head.weight.data_ptr() == lin.weight.data_ptr() and head.norm_weight.data_ptr() == norm.weight.data_ptr() and head.eps == 1e-5
    assert head.bias is None and TokenEmbedding(w).weight is w
