"""-m gpu: bit-exact parity on the integer lattice (tests/helpers.py make_lattice_case): every partial sum of every output is exact in fp32
in any order, so every correct kernel returns ONE value -- the single RNE rounding of the exact sum, bias added as the reference does
(T(T(acc) + b), qmodule.py:221).  Every comparison here is bit equality against `lattice_oracle` (torch's float64 GEMM of the integers on the GPU,
none of this project's kernels), no tolerance.  Outputs and workspaces are NaN-poisoned (helpers.poisoned), so a tile a kernel did not write
cannot pass with the previous launch's result.

The real BASELINE layer shapes (Llama-3-8B, Llama-2-7B in W4 and W3, Llama-3-70B world 1 and its TP = 8 shards, OPT-125M, edge shapes), bf16 and
fp16, at every row count where the routing hands over (ROWS), through the entries the product uses: WQLinear after to_cdna4 (+- bias), WQLinear in
v2 layout (engine cache on / off), gemm_cdna4 (+- sz_half), partial_cdna4, the fused gate / up pair (entry and QuantLlamaMLP), W3, the grouped MoE
entries, the TP = 8 row split summed in fp32, graph replay, the knob-forced variants, fp16 overflow, and split-K under concurrency."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest
import torch

from tests.helpers import (Gen, assert_lattice_equal, check_fused_tail_exact, lattice_bias, lattice_oracle, lattice_weight_f64,
                           make_lattice_case, poisoned, rne_ties)

pytestmark = pytest.mark.gpu

# row counts: every decode / skinny count, then both sides of each hand-over (16 / 32 / 48 / 64-row tiles, the mid-M passes, the 256-row tiles)
ROWS = list(range(1, 25)) + [31, 32, 33, 47, 48, 49, 63, 64, 65, 71, 72, 96, 127, 128, 129, 192, 193, 254, 255, 256, 257, 300, 511, 512, 513, 1024]
ROWS_2048 = ROWS + [2048]

# (name, K, N, bits); the Llama-3-8B and 70B world-1 layers also run 2048 rows (_rows)
LAYERS = [("l3_8b.qkv", 4096, 6144, 4), ("l3_8b.o", 4096, 4096, 4), ("l3_8b.gate", 4096, 14336, 4), ("l3_8b.down", 14336, 4096, 4),
          ("l2_7b.qkv", 4096, 12288, 4), ("l2_7b.gate", 4096, 11008, 4), ("l2_7b.down", 11008, 4096, 4),
          ("l2_7b.qkv.w3", 4096, 12288, 3), ("l2_7b.gate.w3", 4096, 11008, 3), ("l2_7b.down.w3", 11008, 4096, 3),
          ("l3_70b.qkv", 8192, 10240, 4), ("l3_70b.o", 8192, 8192, 4), ("l3_70b.gate", 8192, 28672, 4), ("l3_70b.down", 28672, 8192, 4),
          ("l3_70b.tp8.qkv", 8192, 1280, 4), ("l3_70b.tp8.gate", 8192, 3584, 4), ("l3_70b.tp8.o", 1024, 8192, 4), ("l3_70b.tp8.down", 3584, 8192, 4),
          ("opt_125m.fc1", 768, 3072, 4), ("opt_125m.fc2", 3072, 768, 4)]
EDGE = [("edge.16x128", 128, 16, 4), ("edge.272x128", 128, 272, 4), ("edge.1040x1280", 1280, 1040, 4)]
# gate / up pairs (name, K, F, bits): the fused entry over the 8 + 8 interleaved stream
PAIRS = [("l3_8b.gate_up", 4096, 14336, 4), ("l2_7b.gate_up", 4096, 11008, 4), ("l2_7b.gate_up.w3", 4096, 11008, 3),
         ("l3_70b.gate_up", 8192, 28672, 4), ("l3_70b.tp8.gate_up", 8192, 3584, 4)]
MOE = [(4096, 14336), (14336, 4096)]  # Mixtral-8x7B w1 / w3 and w2, 8 experts
MOE_COUNTS = [0, 1, 9, 255, 256, 257, 543, 2]  # ragged: an empty expert and both sides of the 256-row grouped launch
DTYPES = [torch.bfloat16, torch.float16]
TP_ROW_SPLIT = {"l3_70b.o": 8, "l3_70b.down": 8}

_REACH = {"decode_plan": set(), "gemm_plan": set(), "ties": {"torch.bfloat16": 0, "torch.float16": 0}}


def _rows(name):
    return ROWS_2048 if name.startswith(("l3_8b.", "l3_70b.")) and ".tp8." not in name else ROWS


@pytest.fixture(scope="module", autouse=True)
def _poison():
    with poisoned():
        yield


@pytest.fixture(scope="module")
def eng():
    import llm_awq_amd
    from llm_awq_amd import ops
    e = llm_awq_amd.load_engine()
    ops._capi.lib()
    yield e
    e.cdna4_cache_enable(True)
    e.cdna4_cache_clear()


@pytest.fixture(scope="module")
def ops():
    from llm_awq_amd import ops as o
    return o


# ---------------- one case per shape, shared by both dtypes (the lattice values are exact in bf16 and fp16 alike) ----------------
_shape_cache = {}


def _shape(N, K, bits, Mmax, seed=0):
    """dtype-independent device side of a lattice case: integers, packed weights, the exact fp32 oracle for Mmax rows"""
    from llm_awq_amd.qmodule import pack_intweight, pack_w3c
    key = (N, K, bits, Mmax, seed)
    if key not in _shape_cache:
        _shape_cache.clear()
        torch.cuda.empty_cache()
        c = make_lattice_case(N, K, torch.bfloat16, seed=seed * 1000003 + N * 7 + K + bits, M=Mmax, bits=bits)
        qd = torch.from_numpy(c["q"]).cuda()
        packed = pack_intweight(qd) if bits == 4 else pack_w3c(qd)
        W = lattice_weight_f64(c, "cuda")
        x = c["x"].cuda()
        _y, y32, _t = lattice_oracle(x, c, W=W)
        del W, qd
        _shape_cache[key] = dict(case=c, packed=packed, x=x, y32=y32)
    return _shape_cache[key]


def _typed(sh, dtype):
    c = sh["case"]
    s, z = c["scales"].to(dtype).cuda(), c["scaled_zeros"].to(dtype).cuda()
    return s, z, sh["x"].to(dtype), sh["y32"].to(dtype)


def _note_ties(y32, dtype):
    _REACH["ties"][str(dtype)] += int(rne_ties(y32, dtype).sum().item())


def _plans(L, M, N, K, bits):
    kern, mode, cols = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(0)
    if M <= 8 and bits == 4 and L.awq_w4a16_decode_cdna4_plan(M, N, K, 0, ctypes.byref(kern)) > 0:
        _REACH["decode_plan"].add(kern.value)
    if L.awq_w4a16_gemm_cdna4_plan(M, N, bits, ctypes.byref(mode), ctypes.byref(cols)) > 0:
        _REACH["gemm_plan"].add(mode.value)


# ---------------- every layer, every row count, every entry ----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,N,bits", LAYERS + EDGE, ids=[c[0] for c in LAYERS + EDGE])
def test_layer_every_row_count_bit_exact(eng, ops, dtype, name, K, N, bits):
    from llm_awq_amd.qmodule import WQLinear
    rows = _rows(name)
    sh = _shape(N, K, bits, max(rows))
    c = sh["case"]
    s, z, x, yT = _typed(sh, dtype)
    _note_ties(sh["y32"], dtype)
    bias = lattice_bias(dict(c, dtype=dtype), seed=N + K).cuda()
    yTb = yT + bias
    szp = ops.pack_sz_cdna4(s, z, K)
    L = ops._capi.lib()

    def lin(qw, with_bias):
        m = WQLinear(bits, 128, K, N, with_bias, "cuda", dtype=dtype)
        m.qweight, m.scales, m.scaled_zeros = qw, s, z
        if with_bias:
            m.bias = bias
        return m

    try:
        if bits == 3:
            m3 = lin(sh["packed"], False)
            for M in rows:
                xm = x[:M].contiguous()
                _plans(L, M, N, K, 3)
                assert_lattice_equal(ops.forward_w3(xm, sh["packed"], s, z, szp), yT[:M], f"{name} forward_w3 M={M}")
                assert_lattice_equal(ops.forward_w3(xm, sh["packed"], s, z, szp, bias), yTb[:M], f"{name} forward_w3 + bias M={M}")
                assert_lattice_equal(ops.partial_w3(xm, sh["packed"], szp), sh["y32"][:M], f"{name} partial_w3 M={M}")
                assert_lattice_equal(m3(xm), yT[:M], f"{name} WQLinear w3 M={M}")
            return
        c4 = ops.repack_v2_to_cdna4(sh["packed"])
        szh, exact = ops.pack_szh_cdna4(s, z, K)
        assert exact, "the lattice scales are f16-exact: the sz_half path must run"
        m4, m4b = lin(sh["packed"].clone(), False).to_cdna4(), lin(sh["packed"].clone(), True).to_cdna4()
        assert torch.equal(m4.qweight, c4) and m4.szh_cdna4 is not False
        mv2 = lin(sh["packed"], False)
        for M in rows:
            xm = x[:M].contiguous()
            _plans(L, M, N, K, 4)
            want, wantb = yT[:M], yTb[:M]
            assert_lattice_equal(m4(xm), want, f"{name} WQLinear cdna4 M={M}")
            assert_lattice_equal(m4b(xm), wantb, f"{name} WQLinear cdna4 + bias M={M}")
            for on in (True, False):
                eng.cdna4_cache_enable(on)
                assert_lattice_equal(mv2(xm), want, f"{name} WQLinear v2 (engine cache {on}) M={M}")
            eng.cdna4_cache_enable(True)
            assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, None, szp), want, f"{name} gemm_cdna4 M={M}")
            assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, None, szp, sz_half=szh), want, f"{name} gemm_cdna4 sz_half M={M}")
            assert_lattice_equal(ops.partial_cdna4(xm, c4, szp, szh if M <= 8 else None), sh["y32"][:M], f"{name} partial_cdna4 M={M}")
        world = TP_ROW_SPLIT.get(name)
        if world:
            _row_split(ops, sh, dtype, s, z, bias, yT, yTb, world, rows, name)
    finally:
        eng.cdna4_cache_enable(True)
        eng.cdna4_cache_clear()


def _row_split(ops, sh, dtype, s, z, bias, yT, yTb, world, rows, name):
    """the TP row split: every rank's K shard as an fp32 partial, run one after the other on this GPU, summed in fp32 in rank order, rounded once
    by awq_round_bias_f32 -- bit-identical to the unsharded layer"""
    from llm_awq_amd.parallel import shard_row_parallel
    K = sh["case"]["K"]
    shards = []
    for r in range(world):
        q, ss, zz, _k = shard_row_parallel(sh["packed"], s, z, world, r)
        ks = q.shape[1]
        shards.append((ops.repack_v2_to_cdna4(q.contiguous()), ops.pack_sz_cdna4(ss.contiguous(), zz.contiguous(), ks), ks))
    assert sum(k for (_q, _p, k) in shards) == K
    for M in rows:
        acc, k0 = None, 0
        for (q, szp, ks) in shards:
            p = ops.partial_cdna4(sh["x"][:M, k0:k0 + ks].to(dtype).contiguous(), q, szp)
            acc = p if acc is None else acc + p
            k0 += ks
        assert_lattice_equal(ops.round_bias_f32(acc, dtype), yT[:M], f"{name} TP={world} row split M={M}")
        assert_lattice_equal(ops.round_bias_f32(acc, dtype, bias), yTb[:M], f"{name} TP={world} row split + bias M={M}")


# ---------------- fused gate / up ----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,F,bits", PAIRS, ids=[c[0] for c in PAIRS])
def test_gate_up_pair_every_row_count(eng, ops, dtype, name, K, F, bits):
    from llm_awq_amd.fused_mlp import QuantLlamaMLP, interleave_gate_up, interleave_gate_up_w3
    from llm_awq_amd.qmodule import WQLinear
    rows = _rows(name)
    # gate and up: two cases of the same K and the same radius; x of the gate case drives both
    cg = make_lattice_case(F, K, torch.bfloat16, seed=F + K + bits, M=max(rows), bits=bits)
    cu = make_lattice_case(F, K, torch.bfloat16, seed=F + K + bits + 1, M=1, bits=bits, R=cg["R"])
    x = cg["x"].to(dtype).cuda()
    g32 = lattice_oracle(x, cg)[1]
    u32 = lattice_oracle(x, cu)[1]
    gT, uT = g32.to(dtype), u32.to(dtype)
    from llm_awq_amd.qmodule import pack_intweight, pack_w3c
    pk = pack_intweight if bits == 4 else pack_w3c
    bufs = []
    for cc in (cg, cu):
        bufs.append((pk(torch.from_numpy(cc["q"]).cuda()), cc["scales"].to(dtype).cuda(), cc["scaled_zeros"].to(dtype).cuda()))
    (gq, gs, gz), (uq, us, uz) = bufs
    if bits == 4:
        qi, si, zi = interleave_gate_up(gq, uq, gs, us, gz, uz)
        c4 = ops.repack_v2_to_cdna4(qi)
        szh, exact = ops.pack_szh_cdna4(si, zi, K)
        assert exact
    else:
        c4, si, zi = interleave_gate_up_w3(gq, uq, gs, us, gz, uz)
    szp = ops.pack_sz_cdna4(si, zi, K)

    def proj(q, s_, z_, n, k):
        m = WQLinear(bits, 128, k, n, False, "cuda", dtype=dtype)
        m.qweight, m.scales, m.scaled_zeros = q, s_, z_
        return m

    down = WQLinear(bits, 128, F, K, False, "cuda", dtype=dtype)  # (not run: our_llama_mlp is the fused gate / up half of the module)
    mlp = QuantLlamaMLP(proj(gq, gs, gz, F, K), down, proj(uq, us, uz, F, K))
    for M in rows:
        xm = x[:M].contiguous()
        what = f"{name} M={M}"
        if bits == 4:
            check_fused_tail_exact(ops.mlp_gate_up_forward_cdna4(xm, c4, szp, szh), gT[:M], uT[:M], what + " entry sz_half")
            check_fused_tail_exact(ops.mlp_gate_up_forward_cdna4(xm, c4, szp, None), gT[:M], uT[:M], what + " entry sz_packed")
        else:
            check_fused_tail_exact(ops.mlp_gate_up_forward_w3(xm, c4, szp), gT[:M], uT[:M], what + " w3 entry")
        check_fused_tail_exact(mlp.our_llama_mlp(xm), gT[:M], uT[:M], what + " QuantLlamaMLP")


# ---------------- MoE (Mixtral-8x7B shapes, ragged experts) ----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N", MOE, ids=["w1", "w2"])
def test_moe_grouped_ragged(eng, ops, dtype, K, N):
    from llm_awq_amd.fused_mlp import interleave_gate_up
    from llm_awq_amd.qmodule import pack_intweight
    E = len(MOE_COUNTS)
    T = sum(MOE_COUNTS)
    cases = [make_lattice_case(N, K, torch.bfloat16, seed=9000 + 31 * e + K, M=T if e == 0 else 1) for e in range(E)]
    R = min(c["R"] for c in cases)
    xall = cases[0]["x"].clamp(-R, R).to(dtype).cuda()
    qw = torch.stack([ops.repack_v2_to_cdna4(pack_intweight(torch.from_numpy(c["q"]).cuda())) for c in cases])
    s = torch.stack([c["scales"].to(dtype) for c in cases]).cuda()
    z = torch.stack([c["scaled_zeros"].to(dtype) for c in cases]).cuda()
    szp = torch.stack([ops.pack_sz_cdna4(s[e], z[e], K) for e in range(E)])
    szh = torch.stack([ops.pack_szh_cdna4(s[e], z[e], K)[0] for e in range(E)])

    def run(counts, x):
        off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
        want = torch.empty(x.shape[0], N, dtype=dtype, device="cuda")
        lo = 0
        for e, n in enumerate(counts):
            if n:
                want[lo:lo + n] = lattice_oracle(x[lo:lo + n], cases[e])[1].to(dtype)
            lo += n
        for side in (None, szh):
            y = ops.moe_forward_cdna4(x, qw, s, z, szp, off, sz_half=side)
            assert_lattice_equal(y, want, f"moe_forward_cdna4 K={K} N={N} counts={counts} sz_half={side is not None}")
        return off

    run(MOE_COUNTS, xall)
    run([0, 1, 0, 2, 0, 1, 0, 3], xall[:7].contiguous())  # <= 8 sorted rows: the grouped decode launch
    if K == 4096:
        # the fused gate / up of the experts: w1 = these cases, w3 = another set, rows interleaved 8 + 8
        ups = [make_lattice_case(N, K, torch.bfloat16, seed=19000 + 31 * e + K, M=1) for e in range(E)]
        qi, si, zi = [], [], []
        for cg, cu in zip(cases, ups):
            q_, s_, z_ = interleave_gate_up(pack_intweight(torch.from_numpy(cg["q"]).cuda()), pack_intweight(torch.from_numpy(cu["q"]).cuda()),
                                            cg["scales"].to(dtype).cuda(), cu["scales"].to(dtype).cuda(),
                                            cg["scaled_zeros"].to(dtype).cuda(), cu["scaled_zeros"].to(dtype).cuda())
            qi.append(ops.repack_v2_to_cdna4(q_))
            si.append(s_)
            zi.append(z_)
        qi, si, zi = torch.stack(qi), torch.stack(si), torch.stack(zi)
        szpi = torch.stack([ops.pack_sz_cdna4(si[e], zi[e], K) for e in range(E)])
        szhi = torch.stack([ops.pack_szh_cdna4(si[e], zi[e], K)[0] for e in range(E)])
        for counts, x in ((MOE_COUNTS, xall), ([0, 1, 0, 2, 0, 1, 0, 3], xall[:7].contiguous())):
            off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
            gT = torch.empty(x.shape[0], N, dtype=dtype, device="cuda")
            uT = torch.empty_like(gT)
            lo = 0
            for e, n in enumerate(counts):
                if n:
                    gT[lo:lo + n] = lattice_oracle(x[lo:lo + n], cases[e])[1].to(dtype)
                    uT[lo:lo + n] = lattice_oracle(x[lo:lo + n], ups[e])[1].to(dtype)
                lo += n
            for side in (None, szhi):
                y = ops.moe_mlp_gate_up_cdna4(x, qi, si, zi, szpi, off, sz_half=side)
                check_fused_tail_exact(y, gT, uT, f"moe_mlp_gate_up_cdna4 counts={counts} sz_half={side is not None}")


# ---------------- graph replay ----------------
GRAPH_ROWS = [1, 4, 9, 16, 64, 100, 128, 200, 300]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N", [(4096, 4096), (14336, 4096)], ids=["l3_8b.o", "l3_8b.down"])
def test_graph_replay_on_fresh_x(eng, ops, dtype, K, N):
    from llm_awq_amd.qmodule import WQLinear, pack_intweight
    c = make_lattice_case(N, K, torch.bfloat16, seed=N + 3 * K, M=max(GRAPH_ROWS))
    x_fresh = torch.from_numpy(Gen(N + 5 * K).g.integers(-c["R"], c["R"] + 1, size=(max(GRAPH_ROWS), K))).to(dtype)  # (same radius, other values)
    W = lattice_weight_f64(c, "cuda")
    x1, x2 = c["x"].to(dtype).cuda(), x_fresh.cuda()
    want = lattice_oracle(x2, c, W=W)[1].to(dtype)
    del W
    s, z = c["scales"].to(dtype).cuda(), c["scaled_zeros"].to(dtype).cuda()
    qv2 = pack_intweight(torch.from_numpy(c["q"]).cuda())
    m4 = WQLinear(4, 128, K, N, False, "cuda", dtype=dtype)
    m4.qweight, m4.scales, m4.scaled_zeros = qv2.clone(), s, z
    m4.to_cdna4()
    mv2 = WQLinear(4, 128, K, N, False, "cuda", dtype=dtype)
    mv2.qweight, mv2.scales, mv2.scaled_zeros = qv2, s, z
    c4, szp, szh = m4.qweight, m4.sz_cdna4, m4.szh_cdna4
    entries = [("WQLinear cdna4", lambda xx: m4(xx)), ("WQLinear v2", lambda xx: mv2(xx)),
               ("gemm_cdna4", lambda xx: ops.gemm_cdna4(xx, c4, s, z, None, szp)),
               ("gemm_cdna4 sz_half", lambda xx: ops.gemm_cdna4(xx, c4, s, z, None, szp, sz_half=szh))]
    try:
        for M in GRAPH_ROWS:
            for what, f in entries:
                xs = x1[:M].clone()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    f(xs)  # (warm-up off the capture: side buffers, plan verdicts, engine-cache entries)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    ys = f(xs)
                xs.copy_(x2[:M])
                g.replay()
                torch.cuda.synchronize()
                assert_lattice_equal(ys, want[:M], f"graph replay {what} K={K} N={N} M={M}")
                del g
    finally:
        eng.cdna4_cache_clear()


# ---------------- knob-forced variants: one lattice case each ----------------
def _c4_case(ops, N, K, dtype, M, seed):
    from llm_awq_amd.qmodule import pack_intweight
    c = make_lattice_case(N, K, torch.bfloat16, seed=seed, M=M)
    s, z = c["scales"].to(dtype).cuda(), c["scaled_zeros"].to(dtype).cuda()
    c4 = ops.repack_v2_to_cdna4(pack_intweight(torch.from_numpy(c["q"]).cuda()))
    szp = ops.pack_sz_cdna4(s, z, K)
    szh = ops.pack_szh_cdna4(s, z, K)[0]
    x = c["x"].to(dtype).cuda()
    y32 = lattice_oracle(x, c)[1]
    b = lattice_bias(dict(c, dtype=dtype), seed=seed).cuda()
    return c4, s, z, szp, szh, x, y32.to(dtype), y32.to(dtype) + b, b


@pytest.mark.parametrize("dtype", DTYPES)
def test_knob_forced_variants(ops, dtype):
    tune = ops._capi.tune
    # mid-M kernel: every compiled block shape x forced K part counts
    c4, s, z, szp, szh, x, want, wantb, b = _c4_case(ops, 1296, 1536, dtype, 200, 41)
    try:
        tune(midm_min=9, midm_max=255)
        for (wv, ns) in [(8, 1), (4, 1), (4, 2)]:
            for ks in (1, 2, 5):
                tune(midm_waves=wv, midm_ns=ns, midm_ks=ks)
                for M in (9, 33, 100, 200):
                    xm = x[:M].contiguous()
                    assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, b, szp), wantb[:M], f"midm w{wv} ns{ns} ks{ks} M={M} + bias")
                    assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, None, szp, sz_half=szh), want[:M], f"midm w{wv} ns{ns} ks{ks} M={M} szh")
    finally:
        tune(midm=1, midm_waves=0, midm_ns=0, midm_ks=0, midm_min=65, midm_max=128)
    # the streaming decode kernel's ring configurations
    try:
        for (N, K) in [(64, 11008), (128, 4096), (48, 1280), (32, 14336)]:
            c4, s, z, szp, szh, x, want, wantb, b = _c4_case(ops, N, K, dtype, 8, N + K)
            for knobs in [dict(gemvd_waves=4, gemvd_d=4), dict(gemvd_waves=8, gemvd_d=1), dict(gemvd_waves=8, gemvd_d=2), dict(gemvd_waves=8, gemvd_d=4),
                          dict(gemvd_waves=8, gemvd_d=8), dict(gemvd_waves=16, gemvd_d=1), dict(gemvd_waves=16, gemvd_d=2), dict(gemvd_waves=16, gemvd_d=4)]:
                tune(decode_skinny_from=9, **knobs)
                for M in (1, 4, 8):
                    assert_lattice_equal(ops.decode_cdna4(x[:M].contiguous(), c4, szh, b, 0), wantb[:M], f"decode {knobs} N={N} K={K} M={M}")
    finally:
        tune(gemvd_waves=0, gemvd_d=0, decode_skinny_from=0)
    # the prefill tile kernels: v6 on / off at both tile widths, the block-pair K split
    c4, s, z, szp, szh, x, want, wantb, b = _c4_case(ops, 1296, 1024, dtype, 777, 43)
    try:
        for v6 in (0, 1):
            for tile_n in (256, 128):
                tune(gemm_variant=4 if tile_n == 256 else 3, gemm_tile_n=tile_n, gemm_v6=v6, gemm_splitk=0)
                for M in (256, 300, 777):
                    assert_lattice_equal(ops.gemm_cdna4(x[:M].contiguous(), c4, s, z, b, szp), wantb[:M], f"v6={v6} tile_n={tile_n} M={M} + bias")
                    assert_lattice_equal(ops.gemm_cdna4(x[:M].contiguous(), c4, s, z, None, szp, sz_half=szh), want[:M], f"v6={v6} tile_n={tile_n} M={M}")
    finally:
        tune(gemm_variant=0, gemm_tile_n=0, gemm_v6=1, gemm_splitk=1)
    c4, s, z, szp, szh, x, want, wantb, b = _c4_case(ops, 4096, 1024, dtype, 1536, 47)
    try:
        for lead in (0, 1):
            tune(gemm_v6_pair_min_nit=8, gemm_v6_pair_lead=lead)
            assert ops._capi.lib().awq_w4a16_gemm_cdna4_pair_plan(1536, 4096, 1024) == 1
            assert_lattice_equal(ops.gemm_cdna4(x, c4, s, z, None, szp), want, f"block pair lead={lead}")
            assert_lattice_equal(ops.gemm_cdna4(x, c4, s, z, b, szp), wantb, f"block pair lead={lead} + bias")
        assert ops.pair_lost_count() == 0
    finally:
        tune(gemm_v6_pair=1, gemm_v6_pair_min_nit=64, gemm_v6_pair_lead=1)


# ---------------- fp16 overflow: exact sums beyond 65504 round to +-inf, as torch's rounding does ----------------
def test_fp16_overflow_is_inf(eng, ops):
    from llm_awq_amd.qmodule import pack_intweight, pack_w3c
    dtype = torch.float16
    N, K = 512, 1024
    c = make_lattice_case(N, K, dtype, seed=77, M=300, e0=4, R=4, finite=False)  # (~28 % of the exact sums beyond 65504)
    x = c["x"].cuda()
    y32 = lattice_oracle(x, c)[1]
    want = y32.to(dtype)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any()), "the case must hold both overflowing and finite outputs"
    s, z = c["scales"].cuda(), c["scaled_zeros"].cuda()
    c4 = ops.repack_v2_to_cdna4(pack_intweight(torch.from_numpy(c["q"]).cuda()))
    szp = ops.pack_sz_cdna4(s, z, K)
    szh, exact = ops.pack_szh_cdna4(s, z, K)
    assert exact
    for M in (1, 4, 8, 9, 16, 33, 64, 100, 128, 256, 300):
        xm = x[:M].contiguous()
        assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, None, szp), want[:M], f"fp16 overflow gemm_cdna4 M={M}")
        assert_lattice_equal(ops.gemm_cdna4(xm, c4, s, z, None, szp, sz_half=szh), want[:M], f"fp16 overflow gemm_cdna4 sz_half M={M}")
        if M <= 8:
            assert_lattice_equal(ops.decode_cdna4(xm, c4, szh, None, 0), want[:M], f"fp16 overflow decode M={M}")
        assert_lattice_equal(ops.partial_cdna4(xm, c4, szp), y32[:M], f"fp16 overflow partial M={M}")
    c3 = make_lattice_case(N, K, dtype, seed=78, M=300, bits=3, e0=4, R=8, finite=False)
    x3 = c3["x"].cuda()
    want3 = lattice_oracle(x3, c3)[1].to(dtype)
    assert bool(torch.isinf(want3).any())
    q3 = pack_w3c(torch.from_numpy(c3["q"]).cuda())
    s3, z3 = c3["scales"].cuda(), c3["scaled_zeros"].cuda()
    szp3 = ops.pack_sz_cdna4(s3, z3, K)
    for M in (1, 8, 9, 64, 100, 256, 300):
        assert_lattice_equal(ops.forward_w3(x3[:M].contiguous(), q3, s3, z3, szp3), want3[:M], f"fp16 overflow forward_w3 M={M}")


# ---------------- split-K under concurrency ----------------
SPLIT_SHAPES = [(8192, 4096, 71), (4096, 4096, 64)]  # (K, N, M): a mid-M launch with K parts, a skinny launch with two K parts


def test_two_streams_alternate_split_k_launches(ops):
    L = ops._capi.lib()
    assert all(L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K) > 0 for (K, N, M) in SPLIT_SHAPES), "both shapes must take a K split"
    dtype = torch.bfloat16
    preps = [_c4_case(ops, N, K, dtype, M, K + N) for (K, N, M) in SPLIT_SHAPES]
    Ws = [lattice_weight_f64(make_lattice_case(N, K, torch.bfloat16, seed=K + N, M=1), "cuda") for (K, N, M) in SPLIT_SHAPES]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for it in range(16):
        for j, st in enumerate(streams):
            sel = (it + j) % 2  # the two streams alternate the shapes
            (K, N, M) = SPLIT_SHAPES[sel]
            c4, s, z, szp, _szh, x0, _w, _wb, _b = preps[sel]
            R = int(x0.float().abs().max().item())
            xh = torch.from_numpy(Gen(1000 * it + 10 * j + sel).g.integers(-R, R + 1, size=(M, K))).to(dtype)
            with torch.cuda.stream(st):
                x = xh.cuda(non_blocking=False)
                y = ops.gemm_cdna4(x, c4, s, z, None, szp)
            outs.append((sel, x, y, it, j))
    torch.cuda.synchronize()
    for (sel, x, y, it, j) in outs:
        want = (x.double() @ Ws[sel].t()).float().to(dtype)
        assert_lattice_equal(y, want, f"two streams: iteration {it} stream {j} shape {SPLIT_SHAPES[sel]}")


def test_per_thread_default_stream_never_shares_ticket_words(ops):
    """two threads call awq_w4a16_forward_cdna4 through the C ABI with stream handle 2 (hipStreamPerThread: a different real stream in each
    thread) -- before the fix both keyed the same ticket lane and the reducer could add the other thread's partials"""
    L = ops._capi.lib()
    dtype = torch.bfloat16
    work = []
    for t, (K, N, M) in enumerate(SPLIT_SHAPES):
        c4, s, z, szp, _szh, x0, _w, _wb, _b = _c4_case(ops, N, K, dtype, M, 7 * K + N)
        W = lattice_weight_f64(make_lattice_case(N, K, torch.bfloat16, seed=7 * K + N, M=1), "cuda")
        R = int(x0.float().abs().max().item())
        xs = [torch.from_numpy(Gen(5000 + 100 * t + i).g.integers(-R, R + 1, size=(M, K))).to(dtype).cuda() for i in range(32)]
        ys = [torch.empty(M, N, dtype=dtype, device="cuda") for _ in range(32)]
        wsb = L.awq_w4a16_forward_cdna4_workspace_bytes(M, N, K)
        ws = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device="cuda")
        want = [(x.double() @ W.t()).float().to(dtype) for x in xs]
        work.append((c4, s, z, szp, xs, ys, ws, wsb, M, N, K, want))
    torch.cuda.synchronize()
    errors = []

    def run(w):
        c4, s, z, szp, xs, ys, ws, wsb, M, N, K, _want = w
        try:
            torch.cuda.set_device(0)
            for x, y in zip(xs, ys):
                rc = L.awq_w4a16_forward_cdna4(x.data_ptr(), c4.data_ptr(), s.data_ptr(), z.data_ptr(), szp.data_ptr(), None, y.data_ptr(),
                                               M, N, K, 128, ops._dt(x), ws.data_ptr(), wsb, ctypes.c_void_p(2))
                if rc != 0:
                    errors.append(rc)
                    return
        except Exception as e:  # (reported after the join)
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(w,)) for w in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a thread did not finish its 32 calls"
    torch.cuda.synchronize()
    assert not errors, errors
    for (_c4, _s, _z, _szp, _xs, ys, _ws, _wsb, M, N, K, want) in work:
        for i, (y, w) in enumerate(zip(ys, want)):
            assert_lattice_equal(y, w, f"hipStreamPerThread call {i} of shape {(K, N, M)}")


def test_sweep_reach():
    """what the sweep above reached: the distinct decode kernels and prefill tile modes (host-side plan queries), the ties exercised per dtype"""
    stats = os.environ.get("AWQ_TEST_STATS")
    rec = {"decode_plan_kernels": sorted(_REACH["decode_plan"]), "gemm_plan_modes": sorted(_REACH["gemm_plan"]), "ties": _REACH["ties"]}
    if stats:
        with open(stats, "a") as f:
            f.write(json.dumps({"test": "test_gpu_lattice::reach", **rec}) + "\n")
    if _REACH["gemm_plan"]:  # (the layer sweep ran in this session)
        assert len(_REACH["decode_plan"]) >= 2 and len(_REACH["gemm_plan"]) >= 2, rec
        assert all(v > 0 for v in _REACH["ties"].values()), rec
