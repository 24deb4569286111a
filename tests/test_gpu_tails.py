"""-m gpu: the elementwise tails every token passes through, pinned at the edges of fp16 / bf16 against the float64 / integer restatements of
tests/tail_oracle.py (tests/test_tail_host.py proves on the CPU that those references reject the plausible faults on these very inputs).

  * SiLU * mul: every one of the 65536 gate patterns x 64 up values through awq_silu_mul; a call large enough for a second trip of the grid-stride
    loop (standalone and interleaved); a set of edge gates driven by selector weights (tail_oracle.selector_case) through every fused epilogue.
    Acceptance: the bits of T(s * up) for s at either end of silu_hull -- bit equality wherever the hull is one code (99.6 % of bf16 gates, 99.9 %
    of fp16 gates).
  * fp32 -> T (+ bias in T), awq_round_bias_f32: bit equality with the integer RNE on every rounding tie, overflow, subnormals, specials.
  * RMSNorm: the loop-trip edges of the 256 x 8 kernel, zero / one-hot / tiny / large rows side by side.
Outputs are NaN-poisoned (helpers.poisoned): a store a kernel skipped cannot pass with an earlier launch's result."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tail_oracle as TO
from tests.helpers import poisoned, rmsnorm_uncertainty

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
ROWS = [1, 4, 8, 9, 16, 64, 65, 128, 129, 256, 300]
K_SEL, F_SEL = 512, 256

# the epilogues silu_f32 is inlined into (csrc): every one must have been reached when the module is through
EPILOGUES = {"gemv_dma.epi1", "gemv_dma.epi2", "gemv_cdna4.epi1", "gemv_cdna4.epi2", "gemv_cdna4.norm", "skinny", "midm.unsplit", "midm.splitk",
             "gemm_v6", "gemm_v4n", "util.silu_mul", "util.silu_mul_interleaved"}
_REACH = {}     # label -> calls
_TOOK = {}      # (what, dtype) -> [took lo, took hi]


@pytest.fixture(scope="module", autouse=True)
def _poison():
    with poisoned():
        yield


@pytest.fixture(scope="module")
def ops():
    import llm_awq_amd
    from llm_awq_amd import ops as o
    llm_awq_amd.load_engine()
    o._capi.lib()
    return o


def _reached(label):
    _REACH[label] = _REACH.get(label, 0) + 1


def _accept(out, c_lo, c_hi, what, dtype, gate=None, up=None, pinned=None):
    bad, lo_n, hi_n = TO.tail_check(out, c_lo, c_hi)
    if pinned is not None:
        bad = bad & pinned.to(bad.device)
    t = _TOOK.setdefault((what.split(" ")[0], str(dtype)), [0, 0])
    t[0] += lo_n
    t[1] += hi_n
    if bool(bad.any()):
        idx = torch.nonzero(bad.reshape(-1))[:6].flatten().cpu()
        rows = []
        for i in idx.tolist():
            g = "" if gate is None else f" gate={gate.reshape(-1)[i].item()!r} up={up.reshape(-1)[i].item()!r}"
            rows.append(f"[{i}]{g} got {out.reshape(-1)[i].item()!r} want {c_lo.reshape(-1)[i].item()!r} | {c_hi.reshape(-1)[i].item()!r}")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs outside the acceptance set; " + "; ".join(rows))


# ---------------- SiLU * mul, standalone ----------------
_sweeps = {}


def _sweep(dtype):
    if dtype not in _sweeps:
        _sweeps[dtype] = TO.sweep_accept(dtype, TO.up_values(dtype))
    return _sweeps[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_mul_every_gate_pattern(ops, dtype):
    """all 65536 gates x 64 ups (4 M elements).  Gates of -inf are not pinned (the code computes -inf * 0): what comes out is printed, and must not
    be a finite nonzero value."""
    gate, up, c_lo, c_hi, pinned = _sweep(dtype)
    out = ops.silu_mul(gate.cuda(), up.cuda())
    _reached("util.silu_mul")
    ninf = ~pinned[:, 0]
    o_ninf = out[ninf.cuda()][:, 0].float().cpu()  # up = 1
    print(f"silu_mul {dtype}: gate = -inf, up = 1 -> {o_ninf.tolist()}")
    assert bool((torch.isnan(o_ninf) | torch.isinf(o_ninf) | (o_ninf == 0)).all())
    _accept(out, c_lo.cuda(), c_hi.cuda(), "sweep silu_mul", dtype, gate, up, pinned)
    t = _TOOK[("sweep", str(dtype))]
    print(f"silu_mul {dtype}: of the outputs whose two ends differ, {t[0]} took lo and {t[1]} took hi")


def _trip_tables(dtype):
    g = TO.all_patterns(dtype)
    upv = TO.rne64_to_T(np.full(65536, 1.0 + TO.one_ulp(dtype)), dtype)
    c_lo, c_hi = TO.tail_accept(g, upv)
    pinned = ~(torch.isinf(g.float()) & (g.float() < 0))
    return g.cuda(), upv[0].item(), c_lo.cuda(), c_hi.cuda(), pinned.cuda()


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_mul_second_loop_trip(ops, dtype):
    """16 777 216 + 8 * 257 elements: the grid is capped at 8192 blocks x 256 threads x 8, so the last 2056 elements are a second trip"""
    g, upv, c_lo, c_hi, pinned = _trip_tables(dtype)
    n = TO.SILU_SECOND_TRIP
    idx = torch.arange(n, device="cuda") % 65536
    gate = g[idx]
    up = torch.full((n,), upv, dtype=dtype, device="cuda")
    out = ops.silu_mul(gate, up)
    _accept(out, c_lo[idx], c_hi[idx], "trip silu_mul", dtype, gate, up, pinned[idx])
    assert not bool(torch.isnan(out[TO.SILU_FIRST_TRIP:]).any()), "the second trip left poison"


# ---------------- selector weights: chosen (gate, up) pairs in front of the fused epilogues ----------------
_sel = {}


def _selector(ops, dtype, bits, K=K_SEL, F=F_SEL):
    """device buffers of selector_case in every layout the entries take"""
    from llm_awq_amd.fused_mlp import interleave_gate_up, interleave_gate_up_w3
    from llm_awq_amd.qmodule import pack_intweight, pack_w3c
    key = (dtype, bits, K, F)
    if key in _sel:
        return _sel[key]
    sc = TO.selector_case(K, F, dtype, bits)
    pk = pack_intweight if bits == 4 else pack_w3c
    gq, uq = (pk(torch.from_numpy(sc[n]["q"]).cuda()) for n in ("gate", "up"))
    gs, us = sc["gate"]["scales"].cuda(), sc["up"]["scales"].cuda()
    gz, uz = sc["gate"]["scaled_zeros"].cuda(), sc["up"]["scaled_zeros"].cuda()
    d = {}
    if bits == 4:
        qi, si, zi = interleave_gate_up(gq, uq, gs, us, gz, uz)
        d["c4"] = ops.repack_v2_to_cdna4(qi)
        d["szh"], exact = ops.pack_szh_cdna4(si, zi, K)
        assert exact, "selector scales are exact normal f16 numbers"
        d["c4_stacked"] = ops.repack_v2_to_cdna4(torch.cat([gq, uq], 0).contiguous())
        ss, zs = torch.cat([gs, us], 1).contiguous(), torch.cat([gz, uz], 1).contiguous()
        d["szp_stacked"] = ops.pack_sz_cdna4(ss, zs, K)
        d["szh_stacked"], exact = ops.pack_szh_cdna4(ss, zs, K)
        assert exact
    else:
        d["c4"], si, zi = interleave_gate_up_w3(gq, uq, gs, us, gz, uz)
    d["si"], d["zi"] = si, zi
    d["szp"] = ops.pack_sz_cdna4(si, zi, K)
    _sel[key] = d
    return d


_edge = {}


def _edge_case(dtype, K=K_SEL, F=F_SEL):
    """x [R, K] holding every edge pair, and the acceptance set [R, F] of its rows (computed once per dtype, left unchanged)"""
    if (dtype, K, F) not in _edge:
        g, u = TO.edge_pairs(dtype)
        x = TO.selector_x(g, u, K)
        gg, uu = TO.selector_pairs(x, F)
        c_lo, c_hi = TO.tail_accept(gg, uu)
        _edge[(dtype, K, F)] = dict(x=x.cuda(), gate=gg.cuda(), up=uu.cuda(), c_lo=c_lo.cuda(), c_hi=c_hi.cuda(), R=x.shape[0])
    return _edge[(dtype, K, F)]


def _drive(fn, M, dtype, what, case=None):
    """run fn(x [M, K]) over all rows of the edge case, M at a time (row counts above the case's cycle through it)"""
    e = case or _edge_case(dtype)
    R = e["R"]
    for r0 in range(0, R, M):
        idx = (r0 + torch.arange(M, device="cuda")) % R
        out = fn(e["x"][idx].contiguous())
        _accept(out, e["c_lo"][idx], e["c_hi"][idx], f"{what} M={M} rows {r0}..", dtype, e["gate"][idx], e["up"][idx])


def _decode_kernel(ops, M, n2, K, epi):
    kern = ctypes.c_int(-1)
    assert ops._capi.lib().awq_w4a16_decode_cdna4_plan(M, n2, K, epi, ctypes.byref(kern)) > 0
    return kern.value


def _note_fused_route(ops, M, n2, K, v6=1):
    """which epilogue the fused entry's DEFAULT routing reaches for M rows, where a host-side plan entry says so"""
    if M <= 8:
        _reached("gemv_dma.epi2" if _decode_kernel(ops, M, n2, K, 2) == 0 else "skinny")
    elif M > 128:  # the tile kernels (the mid-M kernel takes at most 128 rows unless forced)
        mode, cols = ctypes.c_int(-1), ctypes.c_int(0)
        assert ops._capi.lib().awq_w4a16_gemm_cdna4_plan(M, n2, 4, ctypes.byref(mode), ctypes.byref(cols)) > 0
        _reached("gemm_v6" if (v6 and M >= 256) else "gemm_v4n")


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_gates_through_the_fused_entries(ops, dtype):
    """awq_w4a16_mlp_gate_up_forward_cdna4 (sz_half and sz_packed) at every row count where the routing hands over; the stacked one-launch entry
    and the decode entry's two fused epilogues at decode row counts"""
    d = _selector(ops, dtype, 4)
    n2 = 2 * F_SEL
    for M in ROWS:
        for side in ("szh", None):
            szh = d["szh"] if side else None
            _drive(lambda x: ops.mlp_gate_up_forward_cdna4(x, d["c4"], d["szp"], szh), M, dtype, f"fused entry sz_half={side is not None}")
        _note_fused_route(ops, M, n2, K_SEL)
    for M in (1, 4, 8):
        _drive(lambda x: ops.mlp_gate_up_cdna4(x, d["c4_stacked"], d["szp_stacked"]), M, dtype, "fused mlp_gate_up_cdna4 (stacked)")
        _reached("gemv_cdna4.epi1")
        _drive(lambda x: ops.decode_cdna4(x, d["c4"], d["szh"], None, 2), M, dtype, "fused decode_cdna4 epilogue 2")
        _reached("gemv_dma.epi2" if _decode_kernel(ops, M, n2, K_SEL, 2) == 0 else "skinny")
    tune = ops._capi.tune
    try:
        tune(decode_skinny_from=9)  # the streaming kernel for every decode row count
        for M in (1, 4, 8):
            assert _decode_kernel(ops, M, n2, K_SEL, 1) == 0 and _decode_kernel(ops, M, n2, K_SEL, 2) == 0
            _drive(lambda x: ops.decode_cdna4(x, d["c4_stacked"], d["szh_stacked"], None, 1), M, dtype, "fused decode_cdna4 epilogue 1 (streaming)")
            _reached("gemv_dma.epi1")
            _drive(lambda x: ops.mlp_gate_up_forward_cdna4(x, d["c4"], d["szp"], d["szh"]), M, dtype, "fused entry (streaming)")
            _reached("gemv_dma.epi2")
    finally:
        tune(decode_skinny_from=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_gates_through_the_knob_forced_variants(ops, dtype):
    """the fused entry under the knobs test_knob_forced_variants enumerates: the mid-M kernel unsplit and with a K split, the skinny kernel, the
    prefill tiles of both kernels at both widths"""
    d = _selector(ops, dtype, 4)
    tune = ops._capi.tune

    def run(M, what):
        for side in ("szh", None):
            szh = d["szh"] if side else None
            _drive(lambda x: ops.mlp_gate_up_forward_cdna4(x, d["c4"], d["szp"], szh), M, dtype, f"fused entry {what} sz_half={side is not None}")

    try:
        tune(midm_min=9, midm_max=255)
        for ks, label in ((1, "midm.unsplit"), (2, "midm.splitk")):
            tune(midm_ks=ks)
            for M in (9, 64, 65, 129, 255):
                run(M, f"midm ks={ks}")
                _reached(label)
    finally:
        tune(midm=1, midm_waves=0, midm_ns=0, midm_ks=0, midm_min=65, midm_max=128)
    try:
        tune(midm=0)
        for M in (9, 16, 64):
            run(M, "midm=0")
            _reached("skinny")
    finally:
        tune(midm=1)
    try:
        for v6 in (0, 1):
            for variant, tile_n in ((4, 256), (3, 128)):
                tune(gemm_variant=variant, gemm_tile_n=tile_n, gemm_v6=v6, gemm_splitk=0)
                for M in (256, 300):
                    run(M, f"gemm_variant={variant} gemm_v6={v6}")
                    _reached("gemm_v6" if v6 else "gemm_v4n")
    finally:
        tune(gemm_variant=0, gemm_tile_n=0, gemm_v6=1, gemm_splitk=1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_gates_through_the_w3_entry(ops, dtype):
    d = _selector(ops, dtype, 3)
    for M in ROWS:
        _drive(lambda x: ops.mlp_gate_up_forward_w3(x, d["c4"], d["szp"]), M, dtype, "fused w3 entry")
        if M <= 8:
            _reached("gemv_cdna4.epi2")
        elif M > 64:
            _reached("gemm_v4n")  # (W3 tiles stay on awq_gemm_v4n.hip: awq_w4a16_gemm_cdna4_narrow_kernel)
            assert ops._capi.lib().awq_w4a16_gemm_cdna4_narrow_kernel(M, 2 * F_SEL, K_SEL, 3, 0, 2) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_gates_through_the_moe_entry(ops, dtype):
    """counts [3, 0, 255, 256, 300]: 814 sorted rows take the grouped tile launch with the tail in its epilogue; [3, 0, 200, 0, 8] (fewer than 256
    sorted rows) take the grouped GEMV / skinny kernels and the interleaved tail as its own launch"""
    d = _selector(ops, dtype, 4)
    e = _edge_case(dtype)
    for counts, label in (([3, 0, 255, 256, 300], "gemm_v6"), ([3, 0, 200, 0, 8], "util.silu_mul_interleaved")):
        E, T = len(counts), sum(counts)
        qw = torch.stack([d["c4"]] * E)
        s, z = torch.stack([d["si"]] * E), torch.stack([d["zi"]] * E)
        szp, szh = torch.stack([d["szp"]] * E), torch.stack([d["szh"]] * E)
        off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
        for r0 in range(0, e["R"], T):
            idx = (r0 + torch.arange(T, device="cuda")) % e["R"]
            x = e["x"][idx].contiguous()
            for side in (None, szh):
                out = ops.moe_mlp_gate_up_cdna4(x, qw, s, z, szp, off, sz_half=side)
                _accept(out, e["c_lo"][idx], e["c_hi"][idx], f"fused moe counts={counts} sz_half={side is not None}", dtype, e["gate"][idx], e["up"][idx])
        assert (T >= 256) == (label == "gemm_v6")
        _reached(label)


@pytest.mark.parametrize("dtype", DTYPES)
def test_interleaved_tail_second_loop_trip(ops, dtype):
    """silu_mul_interleaved_kernel's grid-stride loop: 255 sorted rows (below the grouped tile launch) x n2 = 131 616 columns are 2 097 630 output
    octets, 478 more than the capped grid covers in one trip.  K = 128: each row holds 64 (gate, up) pairs, the columns cycle through them."""
    K, n2, T = 128, 131616, 255
    assert T * (n2 // 16) > TO.SILU_FIRST_TRIP // 8
    F = n2 // 2
    d = _selector(ops, dtype, 4, K, F)
    g = TO.all_patterns(dtype)
    fin = torch.isfinite(g.float())
    gates = g[fin][torch.arange(T * 64) * 3 % int(fin.sum())]           # a spread of finite gate patterns
    ups = TO.rne64_to_T(np.full(T * 64, -(2.0 - TO.one_ulp(dtype))), dtype)
    x = TO.selector_x(gates, ups, K)
    assert x.shape == (T, K)
    gg, uu = TO.selector_pairs(x, 64)                                    # [T, 64]: column n of the output holds pair n mod 64
    c_lo, c_hi = (t.cuda() for t in TO.tail_accept(gg, uu))
    col = torch.arange(F, device="cuda") % 64
    counts = [100, 0, 155]
    E = len(counts)
    qw = torch.stack([d["c4"]] * E)
    s, z = torch.stack([d["si"]] * E), torch.stack([d["zi"]] * E)
    szp = torch.stack([d["szp"]] * E)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    out = ops.moe_mlp_gate_up_cdna4(x.cuda(), qw, s, z, szp, off)
    _reached("util.silu_mul_interleaved")
    _accept(out, c_lo[:, col], c_hi[:, col], "trip interleaved tail", dtype, gg.cuda()[:, col], uu.cuda()[:, col])
    del _sel[(dtype, 4, K, F)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_gates_through_the_fused_rmsnorm_entry(ops, dtype):
    """awq_w4a16_rmsnorm_forward_cdna4 with fused_gate_up, M <= 4, gamma exactly 1.  The normalised row has mean square 1, so a row of chosen gates can
    keep its values only where rsqrt(mean + eps) is exactly a power of two WHATEVER the gates: with eps = 1 and every |x| < 2^-13 the mean is below
    half an ulp of 1, mean + eps = 1 in fp32 in any summation order and the normalised row is x itself (checked with the oracle's rmsnorm).  That
    is the edge gates of magnitude below 2^-13 -- +-0, the smallest subnormals, the tiny gates with a subnormal silu; larger gates cannot be put in
    front of this epilogue exactly and are left to the other entries (the epilogue code is the same silu_f32)."""
    from oracle import awq_oracle as O
    K, F = K_SEL, F_SEL
    g = TO.edge_gates(dtype)
    g = g[g.double().abs() < 2.0 ** -13]
    ups = TO.rne64_to_T(np.array([TO.smallest_normal(dtype), -(1.0 + TO.one_ulp(dtype)) * 2.0 ** -14, 2.0 ** -15]), dtype)
    x = TO.selector_x(g.repeat_interleave(3), ups.repeat(g.numel()), K)
    gamma = torch.ones(K, dtype=dtype)
    assert torch.equal(O.rmsnorm(x, gamma, 1.0).view(torch.int16), x.view(torch.int16)), "the normalised row must be x exactly"
    gg, uu = TO.selector_pairs(x, F)
    c_lo, c_hi = TO.tail_accept(gg, uu)
    case = dict(x=x.cuda(), gate=gg.cuda(), up=uu.cuda(), c_lo=c_lo.cuda(), c_hi=c_hi.cuda(), R=x.shape[0])
    d = _selector(ops, dtype, 4)
    gm = gamma.cuda()
    for M in (1, 2, 4):
        _drive(lambda xx: ops.rmsnorm_forward_cdna4(xx, gm, 1.0, d["c4_stacked"], d["szp_stacked"], None, fused_gate_up=True), M, dtype,
               "fused rmsnorm + gate/up", case)
        _reached("gemv_cdna4.norm")


def test_every_epilogue_was_reached():
    """runs last: the routes the tests above took (host-side plan entries where one exists, the forced knob otherwise) cover every place silu_f32 is
    inlined into, and the share of lo / hi outcomes is printed"""
    print("epilogues reached:", dict(sorted(_REACH.items())))
    print("lo / hi outcomes where the two ends differ:", {f"{k[0]} {k[1]}": v for k, v in sorted(_TOOK.items())})
    if "gemm_v4n" in _REACH or "midm.splitk" in _REACH:  # (the module ran as a whole)
        assert EPILOGUES <= set(_REACH), sorted(EPILOGUES - set(_REACH))


# ---------------- fp32 -> T rounding (+ bias) ----------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_f32_on_every_tie(ops, dtype):
    p = TO.rounding_patterns(dtype)
    want = TO.rne_to_T(p, dtype)
    for n in (8, p.numel()):
        got = ops.round_bias_f32(p.reshape(-1, n).cuda(), dtype).reshape(-1)
        assert bool((torch.isnan(got).cpu() == torch.isnan(want)).all()), "NaN must stay NaN, nothing else may become NaN"
        ok = TO.bits_equal_or_nan(got, want).cpu()
        assert bool(ok.all()), (int((~ok).sum()), p[~ok][:4].view(torch.int32), got.cpu()[~ok][:4], want[~ok][:4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(4, 8), (300, 264), TO.ROUND_BIG], ids=["n8", "n264", "second-trip"])
def test_round_bias_f32(ops, dtype, m, n):
    """T(T(y) + b): n = 8 (the bias is one octet), n = 264, and 2056 x 4104 = 8 437 824 elements -- a second trip of the loop capped at 4096 blocks"""
    y, b = TO.round_inputs(dtype, m, n), TO.bias_values(dtype, n)
    want = TO.round_bias_ref(y, b, dtype)
    got = ops.round_bias_f32(y.cuda(), dtype, b.cuda())
    ok = TO.bits_equal_or_nan(got, want)
    if not bool(ok.all()):
        i = torch.nonzero(~ok.reshape(-1))[:4].flatten().cpu()
        raise AssertionError((int((~ok).sum()), y.reshape(-1)[i], b[i % n], got.reshape(-1).cpu()[i], want.reshape(-1)[i]))
    if n >= 64:
        off = TO.round_bias_ref(y, torch.roll(b, -8), dtype)
        assert int((~TO.bits_equal_or_nan(off, want)).sum()) > 0, "a bias read one octet off must show on these inputs"


# ---------------- RMSNorm ----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", TO.RMS_K)
def test_rmsnorm_loop_trip_edges(ops, dtype, K):
    """ops.rmsnorm and the extension's layernorm_forward_cuda, M = 5: an all-zero row (exactly +-0, the sign of x * gamma), a one-hot row, rows at
    2^-12, 2^6 and ~200.  Within helpers.rmsnorm_uncertainty of the float64 result: bit equality where the rounding is decided, one ulp of T where
    the last bits of the fp32 rstd decide.  (Rows whose fp32 sum of squares overflows are out of scope.)"""
    import llm_awq_amd
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine as E
    x, gamma = TO.rmsnorm_rows(K, dtype)
    ref = TO.rmsnorm_ref(x, gamma, TO.RMS_EPS)
    unc = rmsnorm_uncertainty(x, gamma, TO.RMS_EPS)
    assert float(unc[0].max()) == 0.0 and bool((ref[0].double() == 0).all())
    y1 = ops.rmsnorm(x.cuda(), gamma.cuda(), TO.RMS_EPS)
    y2 = torch.empty_like(y1)
    E.layernorm_forward_cuda(x.cuda(), gamma.cuda(), y2, TO.RMS_EPS)
    for what, y in (("ops.rmsnorm", y1.cpu()), ("layernorm_forward_cuda", y2.cpu())):
        assert bool(torch.isfinite(y.float()).all()), what
        diff = (y.double() - ref.double()).abs()
        bad = diff > unc
        assert not bool(bad.any()), (what, K, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
        decided = unc == 0
        same = y.view(torch.int16) == ref.view(torch.int16)
        assert bool(same[decided].all()), (what, K, "bits differ where the rounding is decided", torch.nonzero(decided & ~same)[:4].tolist())
