"""Decode attention on the MI355X (csrc/awq_attn_cdna4.hip) against the float64 oracle (tests/attn_oracle.py), through the C ABI
(llm_awq_amd.ops) and through awq_inference_engine installed under the reference module name."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from tests import attn_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine  # the reference's module name (tinychat/models/llama.py)

    return awq_inference_engine


def make(B, H, Hkv, Dh, Lmax, dtype, seed, Bc=None):
    """Random q, k, v (CPU) and FT caches (CPU).  v is centred on 1 so that outputs stay away from zero: the 1-ulp check is then
    a statement about the attention, not about fp32 cancellation."""
    g = torch.Generator().manual_seed(seed)
    Bc = Bc or B
    q = (1.5 * torch.randn(B, H, Dh, generator=g)).to(dtype)
    k = torch.randn(B, Hkv, Dh, generator=g).to(dtype)
    v = (1 + 0.5 * torch.randn(B, Hkv, Dh, generator=g)).to(dtype)
    K = torch.randn(Bc, Hkv, Lmax, Dh, generator=g).to(dtype)
    V = (1 + 0.5 * torch.randn(Bc, Hkv, Lmax, Dh, generator=g)).to(dtype)
    return q, k, v, A.to_ft_k_cache(K), V.contiguous()


def run(q, k, v, kc, vc, lens=None, alibi=None, engine=False, **kw):
    """Kernel call on device copies; returns (out, k_cache after, v_cache after) on the CPU."""
    d = [t.to(DEV) for t in (q, k, v, kc, vc)]
    dl = lens.to(DEV) if lens is not None else None
    da = alibi.to(DEV) if alibi is not None else None
    if engine:
        E = _engine()
        out = E.single_query_attention(d[0], d[1], d[2], d[3], d[4], dl, da, kw["timestep"], kw.get("rotary_embedding_dim", 0),
                                       kw.get("rotary_base", 10000.0), kw.get("rotary_scale", 1.0), kw.get("neox_rotary_style", True))
    else:
        out = ops.single_query_attention(*d, dl, da, **kw)
    torch.cuda.synchronize()
    return out.cpu(), d[3].cpu(), d[4].cpu()


def check_out(out, ref, dtype, rotary):
    assert torch.isfinite(out.float()).all()
    if rotary:
        rel = ((out.double() - ref).norm() / ref.norm()).item()
        assert rel <= REL[dtype], rel
    else:
        err = (out.double() - ref).abs()
        bad = err > A.ulp(ref, dtype)
        assert not bad.any(), (err[bad][:8], ref[bad][:8], int(bad.sum()))


def _cases():
    """Every axis value of the issue's sweep appears at least once (not the cartesian product)."""
    dts = (torch.float16, torch.bfloat16)
    groups = (1, 4, 7, 8)
    batches = (1, 3, 8)
    steps = (0, 1, 63, 64, 65, 1000, 4095)
    rots = ("none", "half_neox", "full_neox", "half_gptj", "full_gptj")
    cases = []
    for i, Dh in enumerate(range(32, 257, 16)):
        for j, dt in enumerate(dts):
            n = 2 * i + j
            cases.append(dict(dtype=dt, Dh=Dh, G=groups[n % 4], B=batches[n % 3], t=steps[n % 7], rot=rots[n % 5],
                              base=(10000.0, 500000.0)[n % 2], scale=(1.0, 0.5, 1.0)[n % 3], alibi=(n % 4 == 3),
                              Lmax=(4096, 1024)[(n // 7) % 2]))
    cases.append(dict(dtype=torch.bfloat16, Dh=128, G=4, B=1, t=32767, rot="full_neox", base=500000.0, scale=1.0, alibi=False,
                      Lmax=32768))
    cases.append(dict(dtype=torch.float16, Dh=64, G=7, B=3, t=32767, rot="none", base=1e4, scale=1.0, alibi=True, Lmax=32768))
    return cases


def _rot(name, Dh):
    if name == "none":
        return 0, True
    r = Dh if name.startswith("full") else Dh // 2
    return r, name.endswith("neox")


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{str(c['dtype'])[6:]}-Dh{c['Dh']}-G{c['G']}-B{c['B']}-t{c['t']}-L{c['Lmax']}-{c['rot']}"
                         + ("-alibi" if c["alibi"] else ""))
def test_oracle_parity(case):
    dt, Dh, G, B, t, Lmax = case["dtype"], case["Dh"], case["G"], case["B"], case["t"], case["Lmax"]
    Hkv = 2 if Lmax <= 4096 else 1
    H = G * Hkv
    rot, neox = _rot(case["rot"], Dh)
    q, k, v, kc, vc = make(B, H, Hkv, Dh, Lmax, dt, seed=Dh * 7 + t)
    alibi = (0.05 * torch.rand(H) + 0.01) if case["alibi"] else None
    kw = dict(timestep=t, rotary_embedding_dim=rot, rotary_base=case["base"], rotary_scale=case["scale"], neox_rotary_style=neox)
    ref, k_rot, _ = A.decode(q, k, v, kc, vc, None, alibi, t, rot, case["base"], case["scale"], neox)
    for engine in (False, True):
        out, _, _ = run(q, k, v, kc, vc, None, alibi, engine=engine, **kw)
        check_out(out, ref, dt, rot > 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("t,Lmax,rot", [(70, 128, 0), (300, 128, 64), (5000, 4096, 128), (0, 64, 128), (40, 64, 0)])
def test_cache_contract(dtype, t, Lmax, rot):
    B, Hkv, G, Dh = 2, 2, 4, 128
    q, k, v, kc, vc = make(B, G * Hkv, Hkv, Dh, Lmax, dtype, seed=t + Lmax)
    kw = dict(timestep=t, rotary_embedding_dim=rot, rotary_base=10000.0, rotary_scale=1.0, neox_rotary_style=True)
    ref, k_rot, _ = A.decode(q, k, v, kc, vc, None, None, t, rot, 10000.0, 1.0, True)
    out, kc1, vc1 = run(q, k, v, kc, vc, **kw)
    check_out(out, ref, dtype, rot > 0)
    # poison every position that is not read: past tlength, and before first_step in circular mode
    first = max(0, t + 1 - Lmax)
    read = set(p % Lmax for p in range(first, t + 1))
    unread = [i for i in range(Lmax) if i not in read]
    kcp, vcp = kc.clone(), vc.clone()
    if unread:
        kcp[:, :, :, unread, :] = float("nan")
        vcp[:, :, unread, :] = float("nan")
    outp, kc2, vc2 = run(q, k, v, kcp, vcp, **kw)
    assert torch.isfinite(outp.float()).all()
    assert torch.equal(outp.view(torch.int16), out.view(torch.int16))
    ti = t % Lmax
    for b in range(B):
        for h in range(Hkv):
            assert torch.equal(vc1[b, h, ti].view(torch.int16), v[b, h].view(torch.int16))
            kw_ = A.k_cache_rows(kc1, b, h, [ti])[0]
            if rot == 0 or t == 0:
                assert torch.equal(kw_.view(torch.int16), k[b, h].view(torch.int16))
            else:
                # one ulp of T, plus what one fp32 ulp of the angle (pow / cos / sin of the kernel vs numpy) moves the pair by
                err = (kw_.double() - k_rot[b, h].double()).abs()
                assert (err <= A.ulp(k_rot[b, h].double(), dtype) + A.angle_slack(k[b, h], t, rot, 10000.0, 1.0, True)).all()
    # every other byte unchanged
    mk = torch.ones(Lmax, dtype=torch.bool)
    mk[ti] = False
    assert torch.equal(kc1[:, :, :, mk, :].view(torch.int16), kc[:, :, :, mk, :].view(torch.int16))
    assert torch.equal(vc1[:, :, mk, :].view(torch.int16), vc[:, :, mk, :].view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layouts_gqa_fused_and_lengths(dtype):
    B, Bc, Hkv, G, Dh, Lmax, t = 3, 5, 2, 4, 128, 2048, 1500
    H = G * Hkv
    q, k, v, kc, vc = make(B, H, Hkv, Dh, Lmax, dtype, seed=11, Bc=Bc)
    kw = dict(timestep=t, rotary_embedding_dim=Dh, rotary_base=10000.0, rotary_scale=1.0, neox_rotary_style=True)
    ref, _, _ = A.decode(q, k, v, kc, vc, None, None, t, Dh, 10000.0, 1.0, True)
    # separate GQA tensors (llama.py) at B < cache batch
    out, kc1, vc1 = run(q, k, v, kc, vc, engine=True, **kw)
    check_out(out, ref, dtype, True)
    assert torch.equal(kc1[B:].view(torch.int16), kc[B:].view(torch.int16)) and torch.equal(vc1[B:].view(torch.int16), vc[B:].view(torch.int16))
    # views of one fused qkv tensor (fused_attn.py): batch stride (H + 2 Hkv) Dh for all three
    qkv = torch.cat([q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], 1).to(DEV)
    qv = qkv[:, :H * Dh].view(B, H, Dh)
    kv_ = qkv[:, H * Dh:(H + Hkv) * Dh].view(B, Hkv, Dh)
    vv = qkv[:, (H + Hkv) * Dh:].view(B, Hkv, Dh)
    E = _engine()
    outf = E.single_query_attention(qv, kv_, vv, kc.to(DEV), vc.to(DEV), None, None, t, Dh, 10000.0, 1.0, True).cpu()
    assert torch.equal(outf.view(torch.int16), out.view(torch.int16))
    # per-row lengths equal per-row single calls
    lens = torch.tensor([3, 1500, 700], dtype=torch.int32)
    outl, _, _ = run(q, k, v, kc, vc, lens=lens, engine=True, **kw)
    for b in range(B):
        kwb = dict(kw, timestep=int(lens[b]))
        ob, _, _ = run(q[b:b + 1], k[b:b + 1], v[b:b + 1], kc[b:b + 1].contiguous(), vc[b:b + 1].contiguous(), **kwb)
        refb, _, _ = A.decode(q[b:b + 1], k[b:b + 1], v[b:b + 1], kc[b:b + 1], vc[b:b + 1], None, None, int(lens[b]), Dh, 10000.0, 1.0, True)
        check_out(outl[b:b + 1], refb, dtype, True)
        check_out(ob, refb, dtype, True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_loop_matches_causal_attention(dtype):
    """llama.py:230-243's positional call for 64 steps, k and v appended by the kernel itself (no rotary: full causal attention
    over the steps so far is then the exact reference)."""
    B, Hkv, G, Dh, Lmax, T = 2, 2, 4, 128, 128, 64
    H = G * Hkv
    E = _engine()
    g = torch.Generator().manual_seed(5)
    Q = (1.5 * torch.randn(T, B, H, Dh, generator=g)).to(dtype)
    K = torch.randn(T, B, Hkv, Dh, generator=g).to(dtype)
    V = (1 + 0.5 * torch.randn(T, B, Hkv, Dh, generator=g)).to(dtype)
    kc = torch.zeros(B, Hkv, Dh // 8, Lmax, 8, dtype=dtype, device=DEV)
    vc = torch.zeros(B, Hkv, Lmax, Dh, dtype=dtype, device=DEV)
    for t in range(T):
        out = E.single_query_attention(Q[t].to(DEV), K[t].to(DEV), V[t].to(DEV), kc, vc, None, None, t, 0, 10000.0, 1.0, True).cpu()
        for b in range(B):
            for h in range(H):
                kvh = h // G
                ref = A.causal_attention(Q[:t + 1, b, h], K[:t + 1, b, kvh], V[:t + 1, b, kvh])[t]
                err = (out[b, h].double() - ref).abs()
                # the oracle's softmax has no 1e-6 in its denominator: one ulp plus that relative 1e-6
                assert (err <= A.ulp(ref, dtype) + 2e-6 * ref.abs()).all(), (t, b, h, err.max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_graph_replay_with_device_lengths(dtype):
    B, Hkv, G, Dh, Lmax, T_UB = 2, 2, 4, 128, 4096, 3000
    H = G * Hkv
    E = _engine()
    q, k, v, kc, vc = make(B, H, Hkv, Dh, Lmax, dtype, seed=3)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    kc_g, vc_g = kc.to(DEV), vc.to(DEV)
    kc_e, vc_e = kc.to(DEV), vc.to(DEV)
    lens = torch.tensor([100, 2000], dtype=torch.int32, device=DEV)
    args = (None, T_UB, Dh, 10000.0, 1.0, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        E.single_query_attention(dq, dk, dv, kc_g.clone(), vc_g.clone(), lens, *args)  # warm-up (allocator pools)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = E.single_query_attention(dq, dk, dv, kc_g, vc_g, lens, *args)
    for step in range(4):
        lens.copy_(torch.tensor([100 + 300 * step, 2000 + 250 * step], dtype=torch.int32))
        graph.replay()
        out_e = E.single_query_attention(dq, dk, dv, kc_e, vc_e, lens, *args)
        torch.cuda.synchronize()
        assert torch.equal(out_g.view(torch.int16), out_e.view(torch.int16)), step
        assert torch.equal(kc_g.view(torch.int16), kc_e.view(torch.int16)) and torch.equal(vc_g.view(torch.int16), vc_e.view(torch.int16))
    # two eager calls are bit-identical
    o1 = E.single_query_attention(dq, dk, dv, kc_e, vc_e, lens, *args)
    o2 = E.single_query_attention(dq, dk, dv, kc_e, vc_e, lens, *args)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layernorm_forward_cuda_export(dtype):
    E = _engine()
    for shape in ((5, 4096), (2, 3, 1024)):
        x = torch.randn(*shape, device=DEV).to(dtype)
        w = (1 + 0.1 * torch.randn(shape[-1], device=DEV)).to(dtype)
        out = torch.empty_like(x)
        assert E.layernorm_forward_cuda(x, w, out, 1e-6) is None
        ref = E.rmsnorm(x, w, 1e-6)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


def test_fp32_is_refused_clearly():
    E = _engine()
    q = torch.randn(1, 8, 128, device=DEV)
    k = torch.randn(1, 2, 128, device=DEV)
    kc = torch.zeros(1, 2, 16, 64, 8, device=DEV)
    vc = torch.zeros(1, 2, 64, 128, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        E.single_query_attention(q, k, k, kc, vc, None, None, 3)
