"""gpu: the AWQ quantisation kernels (awq_quantize_group, awq_clip_search) and what is built on them (llm_awq_amd.quantize,
WQLinear.quantize_linear) against the torch-CPU oracle of tests/awq_quant_oracle.py.  The quantiser's outputs are compared bit for bit; the clip
search's error table is held to the fp64 oracle within the tolerance of tests/awq_quant_cases.py and its choice is exact wherever the oracle
is decisive."""
import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops, quantize
from llm_awq_amd.qmodule import WQLinear
from tests import awq_quant_cases as C
from tests import awq_quant_oracle as QO
from tests.conftest import as_t

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
OUTPUTS = ("w_fake", "scales", "scaled_zeros", "zeros")


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(QO.bits(got), QO.bits(want))


def _check_quant(got: dict, want: dict, layout=None):
    for name in OUTPUTS:
        if name in got:
            assert _same(got[name], want[name]), name
    if "qweight" in got:
        assert torch.equal(got["qweight"].cpu(), want["qweight_" + layout]), "qweight " + layout


def _variant(N, K, dtype, variant):
    cs = C.make_col_scale(K, dtype) if "cs" in variant else None
    cm = C.make_clip_max(N, K, dtype) if "clip" in variant else None
    return cs, cm


@pytest.mark.parametrize("variant", ["plain", "cs", "clip", "cs+clip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", C.QUANT_SHAPES, ids=lambda s: "n%d-k%d" % s)
def test_quantize_pack_equals_the_torch_composition_bit_for_bit(shape, dtype, variant):
    N, K = shape
    w = C.make_weight(N, K, dtype)
    cs, cm = _variant(N, K, dtype, variant)
    want = QO.quantize_group(w, cs, cm, 4)
    dev = lambda t: None if t is None else t.to(DEV)
    v2 = ops.quantize_pack(dev(w), dev(cs), dev(cm), 4, "v2", w_fake=True, zeros=True)
    _check_quant(v2, want, "v2")
    c4 = ops.quantize_pack(dev(w), dev(cs), dev(cm), 4, "cdna4", scales=False, scaled_zeros=False)
    assert set(c4) == {"qweight"}
    _check_quant(c4, want, "cdna4")
    assert torch.equal(c4["qweight"], ops.repack_v2_to_cdna4(v2["qweight"]))
    assert int((want["intweight"] < 0).sum() + (want["intweight"] > 15).sum()) == 0  # (what the low four bits keep is the whole integer here)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_quantize_pack_three_bit_grid_and_strided_rows(dtype):
    N, K = 48, 384
    w = C.make_weight(N, K, dtype)
    cs, cm = _variant(N, K, dtype, "cs+clip")
    got = ops.quantize_pack(w.to(DEV), cs.to(DEV), cm.to(DEV), 3, w_fake=True, zeros=True, qweight=False)
    _check_quant(got, QO.quantize_group(w, cs, cm, 3))
    with pytest.raises(RuntimeError):
        ops.quantize_pack(w.to(DEV), n_bit=3)  # a packed 3-bit output is not produced here
    # a column slice of a wider matrix: row stride K + 128, the columns in front are NaN
    wide = torch.full((N, K + 128), float("nan"), dtype=dtype, device=DEV)
    wide[:, 128:] = w.to(DEV)
    view = wide[:, 128:]
    assert not view.is_contiguous()
    got = ops.quantize_pack(view, n_bit=4, layout="cdna4", w_fake=True, zeros=True)
    _check_quant(got, QO.quantize_group(w, None, None, 4), "cdna4")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("only", [("w_fake",), ("scales", "scaled_zeros"), ("zeros",), ("qweight",), ("scales",)])
def test_only_requested_outputs_are_written_and_nothing_around_them(only, dtype):
    """every requested output lies inside a sentinel-filled buffer: the launch writes all of it and not one element in front of or behind it"""
    N, K = 48, 384
    G, gpad = K // 128, 8
    w = C.make_weight(N, K, dtype)
    want = QO.quantize_group(w, None, None, 4)
    shapes = {"w_fake": (N, K), "scales": (gpad, N), "scaled_zeros": (gpad, N), "zeros": (N, G), "qweight": (N // 4, K)}
    guard, arenas, outs = 64, {}, {}
    for name in only:
        dt = torch.int16 if name == "qweight" else dtype
        numel = int(np.prod(shapes[name]))
        arena = torch.full((numel + 2 * guard,), 0x7B7B, dtype=torch.int16, device=DEV)
        arenas[name] = arena
        outs[name] = arena[guard:guard + numel].view(dt).view(shapes[name])
    kw = {name: outs.get(name, False) for name in shapes}
    got = ops.quantize_pack(w.to(DEV), n_bit=4, layout="cdna4", **kw)
    assert set(got) == set(only)
    _check_quant(got, want, "cdna4")
    for name, arena in arenas.items():
        assert bool((arena[:guard] == 0x7B7B).all()) and bool((arena[-guard:] == 0x7B7B).all()), name
        assert got[name].data_ptr() == outs[name].data_ptr()


def _guarded(shape, dtype, guard=64):
    arena = torch.full((int(np.prod(shape)) + 2 * guard,), 0x7B7B, dtype=torch.int16, device=DEV)
    return arena, arena[guard:-guard].view(dtype).view(shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_partial_row_tiles(dtype):
    """any N for the unpacked outputs (5 rows: a third of a 16-row block); N % 8 == 0 is enough for v2 (24 rows: one and a half blocks)"""
    K, G, gpad = 256, 2, 8
    for N, packed in ((5, False), (24, True)):
        w = C.make_weight(N, K, dtype, 7)
        want = QO.quantize_group(w, None, None, 4)
        shapes = {"w_fake": (N, K), "scales": (gpad, N), "scaled_zeros": (gpad, N), "zeros": (N, G)}
        if packed:
            shapes["qweight"] = (N // 4, K)
        held = {name: _guarded(shape, torch.int16 if name == "qweight" else dtype) for name, shape in shapes.items()}
        got = ops.quantize_pack(w.to(DEV), n_bit=4, layout="v2", **{name: held[name][1] if name in held else False for name in
                                                                    ("w_fake", "scales", "scaled_zeros", "zeros", "qweight")})
        _check_quant(got, want, "v2")
        for name, (arena, _) in held.items():
            assert bool((arena[:64] == 0x7B7B).all()) and bool((arena[-64:] == 0x7B7B).all()), (N, name)
    with pytest.raises(RuntimeError):
        ops.quantize_pack(C.make_weight(24, K, dtype, 7).to(DEV), n_bit=4, layout="cdna4")  # cdna4 tiles need N % 16 == 0


@pytest.mark.parametrize("key", ["f16_a", "bf16_a", "f16_b", "bf16_b"])
def test_quantize_pack_equals_the_reference_outputs(golden, key):
    """tests/golden/from_linear.npz: what the reference's pseudo_quantize_tensor + WQLinear.from_linear made of w0"""
    g = golden("from_linear.npz")
    T = {"f16": torch.float16, "bf16": torch.bfloat16}[key.split("_")[0]]
    got = ops.quantize_pack(as_t(g[key + "_w0"], T).to(DEV), n_bit=4, layout="v2", w_fake=True, zeros=True)
    for name, stored in (("w_fake", "wfake"), ("zeros", "z"), ("scales", "scales"), ("scaled_zeros", "scaled_zeros")):
        assert np.array_equal(QO.bits(got[name]).numpy(), g[f"{key}_{stored}"]), name
    assert np.array_equal(got["qweight"].cpu().numpy(), g[key + "_qweight"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_python_entries_equal_the_oracle(dtype):
    N, K = 48, 384
    w = C.make_weight(N, K, dtype)
    want = QO.quantize_group(w, None, None, 4)
    fake, s, z = quantize.pseudo_quantize_tensor(w.to(DEV), n_bit=4, zero_point=True, q_group_size=128, get_scale_zp=True)
    assert _same(fake, want["w_fake"]) and _same(s, want["s"]) and _same(z, want["zeros"])
    w4 = w.to(DEV).reshape(N, 1, K // 128, 128)  # the shape auto_clip_layer hands to it
    f4 = quantize.pseudo_quantize_tensor(w4, n_bit=4, zero_point=True, q_group_size=128)
    assert f4.shape == w4.shape and _same(f4.reshape(N, K), want["w_fake"])
    inplace = w.to(DEV).clone()
    assert quantize.pseudo_quantize_tensor(inplace, n_bit=4, q_group_size=128, inplace=True) is inplace and _same(inplace, want["w_fake"])
    want3 = QO.quantize_group(w, None, None, 3)
    assert _same(quantize.pseudo_quantize_tensor(w.to(DEV), n_bit=3, q_group_size=128), want3["w_fake"])
    cs = C.make_col_scale(K, dtype)
    out = torch.empty(N, K, dtype=dtype, device=DEV)
    assert quantize.fake_quant_scaled(w.to(DEV), cs.to(DEV), out=out) is out
    assert _same(out, QO.quantize_group(w, cs, None, 4)["w_fake"])
    with pytest.raises(TypeError):
        ops.quantize_pack(torch.zeros(16, 128, device=DEV))  # fp32


@pytest.mark.parametrize("layout", ["cdna4", "v2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_quantize_linear_equals_the_from_linear_route(dtype, layout):
    N, K = 48, 384
    w = C.make_weight(N, K, dtype)
    bias = (torch.randn(N) * 0.1).to(dtype)
    lin = torch.nn.Linear(K, N, bias=True, dtype=dtype)
    lin.weight.data, lin.bias.data = w.clone(), bias
    lin = lin.to(DEV)
    got = WQLinear.quantize_linear(lin, 4, 128, layout=layout)
    fake, s, z = QO.O.pseudo_quantize(w, 4, 128)
    lin_fake = torch.nn.Linear(K, N, bias=True, dtype=dtype)
    lin_fake.weight.data, lin_fake.bias.data = fake, bias
    ref = WQLinear.from_linear(lin_fake.to(DEV), 4, 128, False, s.to(DEV), z.to(DEV))
    if layout == "cdna4":
        ref = ref.to_cdna4()
    assert got.layout == ref.layout == layout
    for name in ("qweight", "scales", "scaled_zeros", "bias"):
        assert _same(getattr(got, name), getattr(ref, name)), name
    if layout == "cdna4":
        assert torch.equal(got.sz_cdna4, ref.sz_cdna4)
        assert (got.szh_cdna4 is False) == (ref.szh_cdna4 is False)
        if got.szh_cdna4 is not False:
            assert torch.equal(got.szh_cdna4, ref.szh_cdna4)
    x = torch.randn(3, K).to(dtype).to(DEV)
    assert _same(got(x), ref(x))


# ---- clip search ----

def _run_clip(r, n_bit=4, strided=False):
    w, x = r["w"].to(DEV), r["x"].to(DEV)
    if strided:  # every other row of a twice as tall matrix whose other rows are NaN
        tall = torch.full((2 * x.shape[0], x.shape[1]), float("nan"), dtype=x.dtype, device=DEV)
        tall[::2] = x
        x = tall[::2]
        assert x.stride(0) == 2 * x.shape[1]
    best, idx, err = ops.clip_search(w, x, n_bit, C.N_GRID, C.N_STEPS, return_err=True)
    return best.cpu(), idx.cpu(), err.cpu()


def _check_clip(r, best, idx, err, dtype, label):
    tol = C.TOL[dtype]
    decisive, allowed = C.decisive_cells(r["err64"], tol)
    frac = decisive.float().mean().item()
    assert frac >= C.DECISIVE_FRACTION, "the oracle is not decisive enough for this case"  # (on the oracle, before the kernel is looked at)
    # 1. the choice is the first strict minimum of the kernel's own table
    assert torch.equal(idx, QO.first_strict_min(err))
    # 2. the bits of the oracle's candidate at that index
    want_mv = r["mv"].permute(1, 2, 0).gather(-1, idx.long().unsqueeze(-1)).squeeze(-1)
    assert _same(best, want_mv)
    # 3. the table against fp64
    dev = C.table_deviation(err, r["err64"])
    agree = (idx == r["idx64"]).float().mean().item()
    print(f"{label}: table deviation {dev:.3g} (tol {tol:.3g}), decisive {frac:.4f}, index = fp64 index in {agree:.4f} of the cells")
    assert dev <= tol
    # 4. the fp64 choice on decisive cells, an index within the distance elsewhere
    assert torch.equal(idx[decisive], r["idx64"][decisive])
    assert bool(allowed.gather(-1, idx.long().unsqueeze(-1)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", C.CLIP_SHAPES, ids=lambda s: "n%d-k%d-s%d" % s)
def test_clip_search_against_the_fp64_oracle(shape, dtype):
    r = C.clip_reference(*shape, dtype)
    best, idx, err = _run_clip(r, strided=(shape == C.CLIP_SHAPES[-1]))
    _check_clip(r, best, idx, err, dtype, f"{shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clip_search_three_bit(dtype):
    r = C.clip_reference(*C.N_BIT3_CASE, dtype, 3)
    _check_clip(r, *_run_clip(r, n_bit=3), dtype, f"{C.N_BIT3_CASE} {dtype} n_bit 3")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_rows_table_does_not_depend_on_the_rows_it_is_served_with(dtype):
    N, K, S = C.CLIP_SHAPES[-1]
    r = C.clip_reference(N, K, S, dtype)
    w, x = r["w"].to(DEV), r["x"].to(DEV)
    best, idx, err = ops.clip_search(w, x, 4, C.N_GRID, C.N_STEPS, return_err=True)
    best16, idx16, err16 = ops.clip_search(w[:16].contiguous(), x, 4, C.N_GRID, C.N_STEPS, return_err=True)
    assert torch.equal(QO.bits(err[:16]), QO.bits(err16)) and torch.equal(idx[:16], idx16) and _same(best[:16], best16)
    again = ops.clip_search(w, x, 4, C.N_GRID, C.N_STEPS, return_err=True)
    assert torch.equal(QO.bits(err), QO.bits(again[2]))


def planted_clip_case(dtype):
    """N 16, K 384, S 8.  Cell (4, 0): an outlier m in a column whose activations are all zero, so clipping it is free; the other weights are
    k / 64 with k in -7 .. 8 and m is the T value whose last candidate round_T(m * 0.55) is 8 / 64: at the last step the grid is exactly
    {k / 64} (scale 1 / 64, zero 7) and the error is exactly 0, at every earlier step it is positive.  Group 2: activations all zero.
    Cells (0, 1) / (1, 1): an all-zero and a constant group."""
    gen = torch.Generator().manual_seed(4242)
    w = torch.randn(16, 384, generator=gen) * 0.02
    x = torch.randn(8, 384, generator=gen)
    cand = torch.linspace(0.2255, 0.2290, 400).to(dtype).unique()
    last = (cand.float() * torch.tensor(QO.shrink_factor(C.N_STEPS - 1, C.N_GRID), dtype=torch.float32)).to(dtype)
    m = float(cand[last.float() == 0.125][0])
    w[4, :128] = torch.randint(-7, 9, (128,), generator=gen) / 64.0
    w[4, 0] = -7 / 64.0
    w[4, 41] = m
    x[:, 41] = 0
    x[:, 256:] = 0
    w[0, 128:256] = 0
    w[1, 128:256] = 0.0123
    return w.to(dtype), x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planted_clip_cells(dtype):
    w, x = planted_clip_case(dtype)
    mv, q = QO.clip_candidates(w, 4, C.N_GRID, C.N_STEPS)
    err64 = QO.clip_error_table(w, x, q, torch.float64)
    last = C.N_STEPS - 1
    assert err64[4, 0, last] == 0 and bool((err64[4, 0, :last] > 0).all()) and float(mv[last, 4, 0]) == 0.125  # (the oracle first)
    assert bool((err64[:, 2] == 0).all()) and bool((err64[0, 1] == 0).all()) and bool((err64[1, 1] == err64[1, 1, 0]).all())
    best, idx, err = (t.cpu() for t in ops.clip_search(w.to(DEV), x.to(DEV), 4, C.N_GRID, C.N_STEPS, return_err=True))
    assert idx[4, 0] == last and err[4, 0, last] == 0 and _same(best[4, 0], mv[last, 4, 0])
    assert bool((err[:, 2] == 0).all()) and bool((idx[:, 2] == 0).all()) and _same(best[:, 2], mv[0, :, 2])
    assert bool((err[0, 1] == 0).all()) and idx[0, 1] == 0 and float(best[0, 1]) == 0.0
    assert bool((err[1, 1] == err[1, 1, 0]).all()) and idx[1, 1] == 0 and _same(best[1, 1], mv[0, 1, 1])
    assert torch.equal(idx, QO.first_strict_min(err))
    assert C.table_deviation(err, err64) <= C.TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clip_search_and_quantiser_replay_as_one_graph(dtype):
    N, K, S = 48, 384, 64
    r = C.clip_reference(N, K, S, dtype)
    w_static, x = torch.zeros(N, K, dtype=dtype, device=DEV), r["x"].to(DEV)

    def step():
        best, idx = ops.clip_search(w_static, x, 4, C.N_GRID, C.N_STEPS)
        out = ops.quantize_pack(w_static, clip_max=best, n_bit=4, layout="cdna4", zeros=True)
        return best, idx, out

    w_static.copy_(C.make_weight(N, K, dtype, 3, True).to(DEV))
    step()  # (first launches outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g_best, g_idx, g_out = step()
    torch.cuda.current_stream().wait_stream(side)
    w_static.copy_(r["w"].to(DEV))  # new weights: the replay must compute, not remember
    graph.replay()
    torch.cuda.synchronize()
    best, idx, out = step()
    assert _same(g_best, best) and torch.equal(g_idx, idx)
    for name in out:
        assert torch.equal(QO.bits(g_out[name]), QO.bits(out[name])), name
    want = QO.quantize_group(r["w"], None, best.cpu(), 4)
    _check_quant(g_out, want, "cdna4")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_auto_clip_then_quantize_module_equals_the_oracle_composition(dtype):
    N, K, S = 48, 384, 64
    r = C.clip_reference(N, K, S, dtype)
    w2 = C.make_weight(32, K, dtype, 5, True)

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up = torch.nn.Linear(K, N, bias=False, dtype=dtype)
            self.inner = torch.nn.Sequential(torch.nn.Linear(K, 32, bias=True, dtype=dtype))
            self.lm_head = torch.nn.Linear(K, 16, bias=False, dtype=dtype)

    blk = Block()
    blk.up.weight.data, blk.inner[0].weight.data = r["w"].clone(), w2.clone()
    blk = blk.to(DEV)
    cfg = {"zero_point": True, "q_group_size": 128}
    feat = r["x"].to(DEV).reshape(2, S // 2, K)  # [batch, tokens, K] as the capture hands it over; 64 tokens: stride 1
    clip_up = quantize.auto_clip_layer(blk.up.weight, feat, 4, cfg)
    assert clip_up.shape == (N, K // 128, 1) and clip_up.dtype == dtype
    decisive, _ = C.decisive_cells(r["err64"], C.TOL[dtype])
    want_mv = r["mv"].permute(1, 2, 0).gather(-1, r["idx64"].long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(QO.bits(clip_up.squeeze(-1))[decisive], QO.bits(want_mv)[decisive])
    quantize.quantize_module(blk, 4, 128, clip_list=[("up", clip_up)], layout="cdna4")
    assert isinstance(blk.up, WQLinear) and isinstance(blk.inner[0], WQLinear) and isinstance(blk.lm_head, torch.nn.Linear)
    for mod, w, clip in ((blk.up, r["w"], clip_up.squeeze(-1).cpu()), (blk.inner[0], w2, None)):
        want = QO.quantize_group(w, None, clip, 4)
        assert mod.layout == "cdna4" and torch.equal(mod.qweight.cpu(), want["qweight_cdna4"])
        assert _same(mod.scales, want["scales"]) and _same(mod.scaled_zeros, want["scaled_zeros"])
    # apply_clip's clamp (auto_clip.py:95-97) followed by an unclipped quantisation is the same thing
    clamped = torch.clamp(r["w"].to(DEV).reshape(N, K // 128, 128), -clip_up, clip_up).reshape(N, K)
    again = ops.quantize_pack(clamped, n_bit=4, layout="cdna4")
    assert torch.equal(again["qweight"], blk.up.qweight) and _same(again["scales"], blk.up.scales)
    y = blk.up(r["x"].to(DEV)[:3])
    assert y.shape == (3, N) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_torch_extension_entries_give_the_same_bits(dtype):
    eng = llm_awq_amd.load_engine()
    N, K, S = 48, 384, 64
    r = C.clip_reference(N, K, S, dtype)
    w, x = r["w"].to(DEV), r["x"].to(DEV)
    cs, cm = C.make_col_scale(K, dtype).to(DEV), C.make_clip_max(N, K, dtype).to(DEV)
    for layout in ("cdna4", "v2"):
        got = dict(zip(("w_fake", "scales", "scaled_zeros", "zeros", "qweight"), eng.quantize_pack(w, cs, cm, 4, layout, True, True, True, True)))
        want = ops.quantize_pack(w, cs, cm, 4, layout, w_fake=True, zeros=True)
        for name in want:
            assert _same(got[name], want[name]), (layout, name)
    assert eng.quantize_pack(w, want_scales=False, want_qweight=False, want_zeros=True)[:3] == (None, None, None)
    best, idx, err = eng.clip_search(w[::2], x[::2], 4, C.N_GRID, C.N_STEPS, True)   # strided rows of both
    want = ops.clip_search(w[::2], x[::2], 4, C.N_GRID, C.N_STEPS, return_err=True)
    assert _same(best, want[0]) and torch.equal(idx, want[1]) and torch.equal(QO.bits(err), QO.bits(want[2]))
    assert eng.clip_search(w, x)[2] is None
    with pytest.raises(RuntimeError):
        eng.clip_search(w, x, n_steps=17)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_auto_clip_layer_takes_the_captured_activations_as_the_reference_hands_them_over(dtype):
    """the reference's capture keeps input_feat on the CPU as [batch, tokens, K] (pre_quant.py:182) and auto_clip_block passes it on with the
    weight on the GPU; 1200 tokens: the subsample takes every second one (through auto_clip_layer itself), and only those move to the device"""
    N, K = 48, 384
    w = C.make_weight(N, K, dtype, 0, True)
    feat = C.make_x(1200, K, dtype, 11).reshape(2, 600, K)
    assert not feat.is_cuda and quantize.clip_token_stride(1200) == 2
    got = quantize.auto_clip_layer(w.to(DEV), feat, 4, {"zero_point": True, "q_group_size": 128})
    assert got.shape == (N, K // 128, 1) and got.dtype == dtype and got.is_cuda
    xs = feat.reshape(-1, K)[::2]
    mv, q = QO.clip_candidates(w, 4, C.N_GRID, C.N_STEPS)
    err64 = QO.clip_error_table(w, xs, q, torch.float64)
    decisive, allowed = C.decisive_cells(err64, C.TOL[dtype])
    assert decisive.float().mean().item() >= C.DECISIVE_FRACTION
    cand = QO.bits(mv.permute(1, 2, 0))                                  # [N, G, steps]
    hit = cand == QO.bits(got.squeeze(-1)).unsqueeze(-1)
    idx64 = QO.first_strict_min(err64)
    assert bool(hit.gather(-1, idx64.long().unsqueeze(-1)).squeeze(-1)[decisive].all())   # the fp64 choice wherever it is decisive
    assert bool((hit & allowed).any(-1).all())                                                 # a candidate within the distance elsewhere
    # the same call on the device's own copy of the same tokens gives the same bits; a wrong subsample (every token, or the odd ones) does not
    same = ops.clip_search(w.to(DEV), xs.to(DEV), 4, C.N_GRID, C.N_STEPS)[0]
    assert _same(got.squeeze(-1), same)
    other = ops.clip_search(w.to(DEV), feat.reshape(-1, K)[1::2].to(DEV), 4, C.N_GRID, C.N_STEPS)[0]
    assert not _same(got.squeeze(-1), other)
