"""not-gpu: the AWQ quantisation entries (awq_quantize_group, awq_clip_search) refuse bad arguments before anything is launched, the wrappers
refuse CPU / fp32 tensors, the oracle of tests/awq_quant_oracle.py reproduces the stored outputs of the reference's own Python, the clip
search's inputs meet the conditions the GPU test relies on, and auto_clip_layer's token subsample rule."""
import ctypes

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi, ops, quantize
from llm_awq_amd.qmodule import WQLinear
from tests import awq_quant_cases as C
from tests import awq_quant_oracle as QO
from tests.conftest import as_t

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _p16():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_quantize_group_argument_validation_without_gpu():
    L = _capi.lib()
    buf, p = _p16()
    q = L.awq_quantize_group  # (w, ldw, col_scale, clip_max, w_fake, scales, scaled_zeros, zeros, qweight, layout, n, k, group, n_bit, dtype, stream)
    outs = (p, p, p, p, p)
    assert q(None, 256, None, None, *outs, 1, 16, 256, 128, 4, 1, None) == -6
    assert q(p, 200, None, None, *outs, 1, 16, 200, 128, 4, 1, None) == -4            # K % 128 != 0
    assert q(p, 256, None, None, *outs, 1, 16, 256, 128, 5, 1, None) == -9            # n_bit 5
    assert q(p, 256, None, None, *outs, 1, 16, 256, 64, 4, 1, None) == -2             # group size
    assert q(p, 256, None, None, *outs, 1, 16, 256, 128, 4, 7, None) == -3            # dtype
    assert q(p, 256, None, None, *outs, 1, 24, 256, 128, 4, 1, None) == -4            # cdna4 with N % 16 != 0
    assert q(p, 256, None, None, *outs, 0, 20, 256, 128, 4, 1, None) == -4            # v2 with N % 8 != 0
    assert q(p, 256, None, None, *outs, 2, 16, 256, 128, 4, 1, None) == -4            # no such layout
    assert q(p, 256, None, None, *outs, 1, 16, 256, 128, 3, 1, None) == -9            # a packed output with n_bit 3
    assert q(p, 128, None, None, *outs, 1, 16, 256, 128, 4, 1, None) == -4            # row stride below K
    assert q(p, 260, None, None, *outs, 1, 16, 256, 128, 4, 1, None) == -4            # row stride % 8
    assert q(p + 2, 256, None, None, *outs, 1, 16, 256, 128, 4, 1, None) == -5
    assert q(p, 256, p + 2, None, *outs, 1, 16, 256, 128, 4, 1, None) == -5
    assert q(p, 256, None, None, p, p, p, p + 1, None, 1, 16, 256, 128, 4, 1, None) == -5
    assert b"4-bit" in L.awq_status_string(-9)


def test_clip_search_argument_validation_without_gpu():
    L = _capi.lib()
    buf, p = _p16()
    c = L.awq_clip_search  # (w, ldw, x, ldx, best_max_val, best_idx, err, n, k, s, group, n_bit, n_grid, n_steps, dtype, stream)
    assert c(p, 256, None, 256, p, p, None, 16, 256, 4, 128, 4, 20, 10, 1, None) == -6
    assert c(p, 256, p, 256, p, None, None, 16, 256, 4, 128, 4, 20, 10, 1, None) == -6
    assert c(p, 200, p, 200, p, p, None, 16, 200, 4, 128, 4, 20, 10, 1, None) == -4   # K % 128 != 0
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 128, 5, 20, 10, 1, None) == -9   # n_bit 5
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 128, 4, 20, 17, 1, None) == -4   # n_steps 17
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 128, 4, 20, 0, 1, None) == -4
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 128, 4, 0, 10, 1, None) == -4    # n_grid
    assert c(p, 256, p, 256, p, p, None, 16, 256, 0, 128, 4, 20, 10, 1, None) == -4   # no token
    assert c(p, 256, p, 256, p, p, None, 0, 256, 4, 128, 4, 20, 10, 1, None) == -4    # no row
    assert c(p, 256, p, 250, p, p, None, 16, 256, 4, 128, 4, 20, 10, 1, None) == -4   # token stride below K
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 64, 4, 20, 10, 1, None) == -2
    assert c(p, 256, p, 256, p, p, None, 16, 256, 4, 128, 4, 20, 10, 2, None) == -3
    assert c(p, 256, p + 2, 256, p, p, None, 16, 256, 4, 128, 4, 20, 10, 1, None) == -5
    assert c(p, 256, p, 256, p, p + 2, None, 16, 256, 4, 128, 4, 20, 10, 1, None) == -5


def test_wrappers_refuse_cpu_and_fp32_tensors():
    w = torch.zeros(16, 128, dtype=torch.float16)
    x = torch.zeros(4, 128, dtype=torch.float16)
    cfg = {"zero_point": True, "q_group_size": 128}
    for call in (lambda: ops.quantize_pack(w), lambda: ops.clip_search(w, x), lambda: quantize.pseudo_quantize_tensor(w, 4, **cfg),
                 lambda: quantize.auto_clip_layer(w, x, 4, cfg), lambda: quantize.fake_quant_scaled(w, torch.ones(128, dtype=torch.float16)),
                 lambda: WQLinear.quantize_linear(torch.nn.Linear(128, 16, bias=False, dtype=torch.float16)),
                 lambda: quantize.quantize_module(torch.nn.Sequential(torch.nn.Linear(128, 16, bias=False, dtype=torch.float16)))):
        with pytest.raises(_capi.AwqNativeError):
            call()
    # what the kernels do not implement raises; nothing falls back to torch
    with pytest.raises(NotImplementedError):
        quantize.pseudo_quantize_tensor(w, n_bit=8, zero_point=True, q_group_size=128)
    with pytest.raises(NotImplementedError):
        quantize.pseudo_quantize_tensor(w, n_bit=4, zero_point=False, q_group_size=128)
    with pytest.raises(NotImplementedError):
        quantize.pseudo_quantize_tensor(w, n_bit=4, zero_point=True, q_group_size=64)
    with pytest.raises(NotImplementedError):
        quantize.auto_clip_layer(w, x, 4, {"zero_point": True, "q_group_size": -1})
    with pytest.raises(NotImplementedError):
        WQLinear.quantize_linear(torch.nn.Linear(128, 16, bias=False, dtype=torch.float16), w_bit=3)


def test_torch_extension_entries_refuse_cpu_tensors():
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    w, x = torch.zeros(16, 128, dtype=torch.float16), torch.zeros(4, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.quantize_pack(w)
    with pytest.raises(RuntimeError, match="GPU"):
        eng.clip_search(w, x)


def test_fp32_cpu_tensors_are_refused_as_cpu_tensors():
    with pytest.raises(_capi.AwqNativeError):
        ops.quantize_pack(torch.zeros(16, 128))
    with pytest.raises(_capi.AwqNativeError):
        ops.clip_search(torch.zeros(16, 128), torch.zeros(2, 128))


@pytest.mark.parametrize("key", ["f16_a", "bf16_a", "f16_b", "bf16_b"])
def test_oracle_piece1_equals_the_reference_outputs(golden, key):
    """tests/golden/from_linear.npz: the reference's pseudo_quantize_tensor + WQLinear.from_linear run on w0"""
    g = golden("from_linear.npz")
    T = DTYPES[key.split("_")[0]]
    o = QO.quantize_group(as_t(g[key + "_w0"], T))
    for name, want in (("w_fake", "wfake"), ("s", "s"), ("zeros", "z"), ("scales", "scales"), ("scaled_zeros", "scaled_zeros")):
        assert np.array_equal(QO.bits(o[name]).numpy(), g[f"{key}_{want}"]), name
    assert np.array_equal(o["qweight_v2"].numpy(), g[key + "_qweight"])


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_oracle_piece1_equals_the_reference_3bit_grid(golden, name):
    g = golden("pseudo_w3.npz")
    o = QO.quantize_group(as_t(g[name + "_w0"], DTYPES[name]), n_bit=3)
    for key, want in (("w_fake", "wfake"), ("s", "s"), ("zeros", "z")):
        assert np.array_equal(QO.bits(o[key]).numpy(), g[f"{name}_{want}"]), key
    assert o["qweight_v2"] is None


@pytest.mark.parametrize("variant", ["plain", "cs", "clip", "cs+clip"])
@pytest.mark.parametrize("n_bit", [4, 3])
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_the_grid_compiled_for_the_host_equals_the_torch_composition(name, n_bit, variant):
    """awq_quantize_group_host: the source text of the kernels' grid (csrc/awq_quant_grid.hpp) compiled for the CPU, bit for bit against the oracle
    on every piece-1 case (planted groups included) -- the arithmetic is checked where there is no GPU"""
    T = DTYPES[name]
    for N, K in C.QUANT_SHAPES:
        G, gpad = K // 128, 8
        w = C.make_weight(N, K, T)
        cs = C.make_col_scale(K, T) if "cs" in variant else None
        cm = C.make_clip_max(N, K, T) if "clip" in variant else None
        want = QO.quantize_group(w, cs, cm, n_bit)
        fake, zeros = torch.full((N, K), 7.0, dtype=T), torch.full((N, G), 7.0, dtype=T)
        scales, sz = torch.full((gpad, N), 7.0, dtype=T), torch.full((gpad, N), 7.0, dtype=T)
        iw = torch.full((N, K), 255, dtype=torch.uint8)
        ptr = lambda t: None if t is None else t.data_ptr()
        st = _capi.lib().awq_quantize_group_host(w.data_ptr(), K, ptr(cs), ptr(cm), fake.data_ptr(), scales.data_ptr(), sz.data_ptr(),
                                                 zeros.data_ptr(), iw.data_ptr(), N, K, 128, n_bit, 0 if T == torch.float16 else 1)
        assert st == 0
        for got, key in ((fake, "w_fake"), (zeros, "zeros"), (scales, "scales"), (sz, "scaled_zeros")):
            assert torch.equal(QO.bits(got), QO.bits(want[key])), (N, K, key)
        assert torch.equal(iw.to(torch.int32), want["intweight"] & 0xF), (N, K)
    L = _capi.lib()
    assert L.awq_quantize_group_host(None, 128, None, None, None, None, None, None, None, 16, 128, 128, 4, 0) == -6
    assert L.awq_quantize_group_host(w.data_ptr(), 200, None, None, None, None, None, None, None, 16, 200, 128, 4, 0) == -4
    assert L.awq_quantize_group_host(w.data_ptr(), 128, None, None, None, None, None, None, None, 16, 128, 128, 5, 0) == -9


def test_shrink_factor_bits():
    want = [0x3f800000, 0x3f733333, 0x3f666666, 0x3f59999a, 0x3f4ccccd, 0x3f400000, 0x3f333333, 0x3f266666, 0x3f19999a, 0x3f0ccccd]
    assert [int(np.float32(QO.shrink_factor(i, 20)).view(np.uint32)) for i in range(10)] == want


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", C.CLIP_SHAPES, ids=lambda s: "n%d-k%d-s%d" % s)
def test_clip_cases_meet_the_conditions_of_the_gpu_test(shape, dtype):
    """one reduction per cell serves every candidate; the fp32 torch evaluation stays within D of fp64 (the kernel gets FACTOR x D) and picks the
    fp64 index wherever the cell is decisive; at least 95 % of the cells are decisive"""
    r = C.clip_reference(*shape, dtype)
    for i in range(C.N_STEPS):
        assert QO.amax_of_clamped_is_clamped_amax(r["w"], r["mv"][i])
    dev = C.table_deviation(r["err32"], r["err64"])
    print(f"{shape} {dtype}: fp32 yardstick deviation {dev:.3g} (D {C.D_F32[dtype]:.3g})")
    assert dev <= 2 * C.D_F32[dtype]   # (the constant was measured on one CPU; another one's fp32 sum order differs)
    decisive, allowed = C.decisive_cells(r["err64"], C.TOL[dtype])
    assert decisive.float().mean().item() >= C.DECISIVE_FRACTION
    idx32 = QO.first_strict_min(r["err32"])
    assert torch.equal(idx32[decisive], r["idx64"][decisive])
    assert bool(allowed.gather(-1, idx32.long().unsqueeze(-1)).all())


def test_the_largest_yardstick_deviation_is_the_stated_D():
    """D is a measurement, not a bound picked far above it: the largest deviation over the cases is within a factor 2 of the constant"""
    for dtype in (torch.float16, torch.bfloat16):
        worst = max(C.table_deviation(r["err32"], r["err64"]) for r in (C.clip_reference(*s, dtype) for s in C.CLIP_SHAPES))
        assert 0.5 * C.D_F32[dtype] <= worst <= 2 * C.D_F32[dtype]


def test_first_strict_min_is_the_references_rule():
    e = torch.tensor([[3.0, 2.0, 2.0, 1.0, 1.0], [2e9, 5e9, float("nan"), 1e9, 3e9], [float("nan"), 4.0, 4.0, 5.0, 3.0]], dtype=torch.float64)
    assert QO.first_strict_min(e).tolist() == [3, 0, 4]


@pytest.mark.parametrize("n_tokens, stride", [(1, 1), (511, 1), (512, 1), (1000, 1), (1024, 2)])
def test_auto_clip_token_subsample_rule(n_tokens, stride):
    assert quantize.clip_token_stride(n_tokens) == stride
    if n_tokens >= 512:  # the reference's own expression (auto_clip.py:23); below 512 tokens its slice step is 0, which raises
        assert n_tokens // 512 == stride
