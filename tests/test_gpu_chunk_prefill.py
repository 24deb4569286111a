"""Chunk prefill on the FT KV cache on the MI355X: attn_prefill_ftcache (csrc/awq_attn_prefill_cdna4.hip) on the needle cases of
tests/attn_prefill_cases.py bit for bit, the same bits as flash_attn_func on the gathered copies for random inputs (and those within the
derived bound of the float64 oracle), rope_kv_store (csrc/awq_attn_chunk_cdna4.hip) bit for bit against two rope calls and the torch
stores, the data flow of llm_awq_amd.fused_attn.QuantLlamaAttentionFused against the composition it replaces, determinism and graph
replay.  The reference tree is not read: its data flow (tinychat/modules/fused_attn.py:248-302, 439-503) is restated here."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_oracle as A
from tests import attn_prefill_cases as C
from tests import attn_prefill_oracle as O
from tests import chunk_prefill_oracle as CP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # tests/test_gpu_attention_prefill.py's, for the eager composition


def _engine():
    return llm_awq_amd.install_as_awq_inference_engine()


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------------
# 1. needle cases: K / V in FT caches with NaN everywhere else, bit equality
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _case(name):
    return C.Case(next(s for s in C.CASES if s["name"] == name))


@pytest.mark.parametrize("kv_start", [0, 3])
@pytest.mark.parametrize("name", [s["name"] for s in C.CASES if s["Dh"] in (64, 128)])
def test_needle_cases_bit_exact_from_the_cache(name, kv_start):
    case = _case(name)
    q, k, v = case.to(DEV)
    B, Sk = k.shape[0], k.shape[1]
    kc, vc = CP.scatter_ft(k, v, B + 1, kv_start + Sk + 5, kv_start)
    assert int(torch.isnan(kc).sum()) == kc.numel() - k.numel() and int(torch.isnan(vc).sum()) == vc.numel() - v.numel()
    out = ops.attn_prefill_ftcache(q, kc, vc, kv_start, Sk, case.scale, case.causal)
    torch.cuda.synchronize()
    assert out.shape == case.target.shape and out.is_contiguous()
    got, want = out.cpu().view(torch.int16), case.target.view(torch.int16)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())


# ------------------------------------------------------------------------------------------------------------------------
# 2. random inputs: the bits of the gathered path, within the derived bound of float64
# ------------------------------------------------------------------------------------------------------------------------
def _random_cases():
    out, n = [], 0
    groups, batches, starts = (1, 4, 8), (1, 3), (0, 3, 17)
    for Sq, Sk in ((1, 65), (33, 64), (64, 64), (65, 130), (130, 700), (32, 1056)):
        for Dh in (64, 128):
            for j, dt in enumerate((torch.float16, torch.bfloat16)):
                # every axis has a period of its own, offset by the dtype: both dtypes and both head dims meet every group size and batch
                m = n + j
                out.append(dict(dtype=dt, Dh=Dh, Sq=Sq, Sk=Sk, G=groups[m % 3], B=batches[(m // 3 + j) % 2], Hkv=(2, 1)[(m // 2) % 2],
                                kv_start=starts[(m + j) % 3], causal=True))
            n += 1
    out.append(dict(dtype=torch.bfloat16, Dh=128, Sq=100, Sk=333, G=4, B=2, Hkv=2, kv_start=3, causal=False))
    return out


def _cid(c):
    return f"{str(c['dtype'])[6:]}-B{c['B']}-G{c['G']}-Hkv{c['Hkv']}-Dh{c['Dh']}-{c['Sq']}x{c['Sk']}-at{c['kv_start']}" + ("" if c["causal"] else "-full")


@functools.lru_cache(maxsize=2)
def _random_data(key):
    """(q, kc, vc, k, v, ref, lim) of one case: inputs with the distributions of tests/test_gpu_attention_prefill.py::make
    (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N), the caches NaN outside the keys, the float64 reference and its bound -- computed once per case."""
    c = dict(key)
    B, Hkv, Dh, Sq, Sk, dt = c["B"], c["Hkv"], c["Dh"], c["Sq"], c["Sk"], c["dtype"]
    H = c["G"] * Hkv
    g = torch.Generator(device=DEV).manual_seed(Sq * 31 + Sk + Dh + H)
    q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dt)
    k = torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV).to(dt)
    v = (1 + 0.5 * torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV)).to(dt)
    lmax = c["kv_start"] + Sk + 5
    lmax += lmax % 64 == 0  # never a multiple of the tile
    kc, vc = CP.scatter_ft(k, v, B + 1, lmax, c["kv_start"])
    ref, Aw, qk = O.attention(q, k, v, None, c["causal"], stats=True)
    lim = O.bound(ref, Aw, qk, dt, Sk, Dh, Dh ** -0.5)
    return q, kc, vc, k, v, ref, lim


@pytest.mark.parametrize("rows", [0, 64, 128, 256])
@pytest.mark.parametrize("c", _random_cases(), ids=_cid)
def test_same_bits_as_the_gathered_path_and_within_the_bound(c, rows):
    q, kc, vc, k, v, ref, lim = _random_data(tuple(sorted(c.items(), key=lambda kv: kv[0])))
    assert vc.shape[2] % 64 != 0
    kg, vg = CP.gather_ft(kc, vc, q.shape[0], c["kv_start"], c["Sk"])
    assert torch.equal(bits(kg), bits(k)) and torch.equal(bits(vg), bits(v))
    try:
        _capi.tune(attn_prefill_rows=rows)  # 0 = the plan's choice
        if rows:
            assert ops.attn_prefill_plan(q.shape[0], q.shape[2], k.shape[2], c["Dh"], c["Sq"], c["Sk"], c["causal"])[0] == rows
        out = ops.attn_prefill_ftcache(q, kc, vc, c["kv_start"], c["Sk"], None, c["causal"])
        nat = ops.flash_attn_func(q, kg, vg, None, c["causal"])
    finally:
        _capi.tune(attn_prefill_rows=0)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(bits(out), bits(nat)), int((bits(out) != bits(nat)).sum())
    err = (out.double() - ref).abs()
    print(f"max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())


def test_strided_q_and_the_engine_binding_agree_with_the_c_abi():
    """q as the slice of a fused qkv tensor (batch and row strides of its own), through both entry points."""
    E = _engine()
    B, S, H, Hkv, Dh, pos = 2, 70, 8, 2, 128, 9
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn(B, S + 2, (H + 2 * Hkv) * Dh, generator=g, device=DEV).to(torch.bfloat16)
    q = qkv[:, :S, :H * Dh].view(B, S, H, Dh)
    k = torch.randn(B, pos + S, Hkv, Dh, generator=g, device=DEV).to(torch.bfloat16)
    v = torch.randn(B, pos + S, Hkv, Dh, generator=g, device=DEV).to(torch.bfloat16)
    kc, vc = CP.scatter_ft(k, v, B, pos + S + 3, 0)
    want = ops.flash_attn_func(q, k, v, None, True)
    assert torch.equal(bits(ops.attn_prefill_ftcache(q, kc, vc, 0, pos + S, None, True)), bits(want))
    assert torch.equal(bits(E.attn_prefill_ftcache(q, kc, vc, 0, pos + S, Dh ** -0.5, True)), bits(want))
    # the chunk alone: keys pos .. pos + S - 1
    want = ops.flash_attn_func(q, k[:, pos:], v[:, pos:], 0.07, True)
    assert torch.equal(bits(E.attn_prefill_ftcache(q, kc, vc, pos, S, 0.07, True)), bits(want))
    with pytest.raises(RuntimeError, match="cache"):
        E.attn_prefill_ftcache(q, kc, vc, pos, S + 4, 0.07, True)  # past the end of the cache


# ------------------------------------------------------------------------------------------------------------------------
# 3. rope_kv_store
# ------------------------------------------------------------------------------------------------------------------------
def fill_ft_caches(kc, vc, k, v, start_pos):
    """fused_attn.py:259-267: v_cache [B, Hkv, L, Dh] <- v, k_cache [B, Hkv, Dh/8, L, 8] <- k at positions start_pos .. start_pos + S."""
    B, S, Hkv, Dh = k.shape
    vc[:B, :, start_pos:start_pos + S, :] = v.transpose(1, 2)
    kc[:B, :, :, start_pos:start_pos + S, :] = k.reshape(B, S, Hkv, Dh // 8, 8).permute(0, 2, 3, 1, 4).contiguous()


def _sentinel(shape, dtype, mul):
    n = math.prod(shape)
    return ((torch.arange(n, device=DEV) * mul + 12345) % 30011).to(torch.int16).view(dtype).reshape(shape).clone()  # finite, positive


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("half_rot", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 63, 65, 200])
def test_rope_kv_store_bits_and_footprint(S, B, half_rot, Dh, dtype):
    E = _engine()
    H, Hkv, L, Bc = 4, 2, 211, 3
    rot = Dh // 2 if half_rot else Dh
    W = (H + 2 * Hkv) * Dh
    for idx, start in enumerate((0, 7, L - S)):
        g = torch.Generator(device=DEV).manual_seed(S * 7 + start + B)
        if idx == 0:
            qkv = torch.randn(B, S, W, generator=g, device=DEV).to(dtype)
        else:  # a strided slice of a wider buffer (NaN around it): row stride, and for the last one a batch stride, of its own
            wide = torch.full((B, S + idx - 1, W + 24), float("nan"), dtype=dtype, device=DEV)
            qkv = wide[:, :S, 8:8 + W]
            qkv.copy_(torch.randn(B, S, W, generator=g, device=DEV))
            assert not qkv.is_contiguous() or B * S == 1
        freqs = (50.0 * torch.randn(S, B, rot, generator=g, device=DEV)).contiguous()  # read flat at (s * B + b) * rot + c
        kc0, vc0 = _sentinel((Bc, Hkv, Dh // 8, L, 8), dtype, 7), _sentinel((Bc, Hkv, L, Dh), dtype, 13)
        # the composition it replaces
        xq, xk, xv = CP.split_qkv(qkv, H, Hkv)
        q_want = E.fused_rope_with_pos_forward_func(xq, freqs, True)
        k_rot = E.fused_rope_with_pos_forward_func(xk, freqs, True)
        kc_want, vc_want = kc0.clone(), vc0.clone()
        fill_ft_caches(kc_want, vc_want, k_rot, xv, start)
        for fn in (ops.rope_kv_store, E.rope_kv_store):
            kc, vc = kc0.clone(), vc0.clone()
            q_out = fn(qkv, freqs, kc, vc, start, H, Hkv)
            torch.cuda.synchronize()
            assert q_out.shape == (B, S, H, Dh) and q_out.is_contiguous()
            assert torch.equal(bits(q_out), bits(q_want))
            assert torch.equal(bits(kc), bits(kc_want)) and torch.equal(bits(vc), bits(vc_want))
            # the footprint, against the sentinel itself
            keep = torch.ones(L, dtype=torch.bool, device=DEV)
            keep[start:start + S] = False
            assert torch.equal(bits(kc[:, :, :, keep]), bits(kc0[:, :, :, keep])) and torch.equal(bits(vc[:, :, keep]), bits(vc0[:, :, keep]))
            assert torch.equal(bits(kc[B:]), bits(kc0[B:])) and torch.equal(bits(vc[B:]), bits(vc0[B:]))
        # the float64 restatement (tests/test_chunk_prefill_host.py): one rounding to T plus fp32 evaluation, as tests/test_gpu_rope.py bounds it
        q_ref, q_mag, k_ref, k_mag, v_new = CP.rope_kv_store(qkv, freqs, kc0, vc0, start, H, Hkv)
        assert not ((q_out.double() - q_ref).abs() > 0.5 * A.ulp(q_ref, dtype) + 4 * 2.0 ** -23 * q_mag).any()
        assert not ((kc.double() - k_ref).abs() > 0.5 * A.ulp(k_ref, dtype) + 4 * 2.0 ** -23 * k_mag).any()
        assert torch.equal(bits(vc), bits(v_new))


def test_rope_kv_store_refuses_what_does_not_fit():
    E = _engine()
    B, S, H, Hkv, Dh, L = 2, 8, 4, 2, 64, 16
    qkv = torch.zeros(B, S, (H + 2 * Hkv) * Dh, dtype=torch.float16, device=DEV)
    fr = torch.zeros(S, B, Dh, device=DEV)
    kc = torch.zeros(B, Hkv, Dh // 8, L, 8, dtype=torch.float16, device=DEV)
    vc = torch.zeros(B, Hkv, L, Dh, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="wrap"):
        E.rope_kv_store(qkv, fr, kc, vc, 9, H, Hkv)
    with pytest.raises(_capi.AwqNativeError):
        ops.rope_kv_store(qkv, fr, kc, vc, 9, H, Hkv)
    with pytest.raises(RuntimeError, match="cache batch"):
        E.rope_kv_store(qkv, fr, kc[:1], vc[:1], 0, H, Hkv)
    with pytest.raises(RuntimeError, match="dtype"):
        E.rope_kv_store(qkv, fr, kc.bfloat16(), vc.bfloat16(), 0, H, Hkv)
    assert not kc.any() and not vc.any()


# ------------------------------------------------------------------------------------------------------------------------
# 4. the module: prompt, second chunk, one decode step
# ------------------------------------------------------------------------------------------------------------------------
def eager_attention(q, k, v, start_pos):
    """fused_attn.py:287-302: repeat_interleave of K / V, [B, H, Sq, Sk] scores / sqrt(Dh), a -inf mask above diagonal start_pos + 1,
    fp32 softmax cast back to T, second matmul.  q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] -> [B, Sq, H, Dh]."""
    B, Sq, H, Dh = q.shape
    G = H // k.shape[2]
    keys = torch.repeat_interleave(k, dim=2, repeats=G).transpose(1, 2)
    values = torch.repeat_interleave(v, dim=2, repeats=G).transpose(1, 2)
    xq = q.transpose(1, 2)
    scores = torch.matmul(xq, keys.transpose(2, 3)) / math.sqrt(Dh)
    if Sq > 1:
        mask = torch.full((1, 1, Sq, k.shape[1]), float("-inf"), device=q.device)
        mask = torch.triu(mask, diagonal=start_pos + 1).type_as(scores)
        scores = scores + mask
    scores = torch.softmax(scores.float(), dim=-1).type_as(xq)
    return torch.matmul(scores, values).transpose(1, 2).contiguous()


def _freqs(start, n, Dh, base=10000.0):
    inv = 1.0 / (base ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    f = torch.outer(torch.arange(start, start + n, device=DEV).float(), inv)
    return torch.cat([f, f], -1)[None].contiguous()  # [1, n, Dh]: one angle per column, rotate-half layout


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


FLOW = dict(B=1, H=8, Hkv=2, Dh=128, L=512, S1=200, S2=56)


def _flow_inputs(dtype):
    """The qkv tensors of the three stages, with the distributions REL is meant for (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N)."""
    B, H, Hkv, Dh = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"]
    mul = torch.cat([torch.full((H * Dh,), 1.5), torch.ones(Hkv * Dh), torch.full((Hkv * Dh,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + Hkv) * Dh), torch.ones(Hkv * Dh)]).to(DEV)
    gg = torch.Generator(device=DEV).manual_seed(3)
    return [(torch.randn(B, S, (H + 2 * Hkv) * Dh, generator=gg, device=DEV) * mul + add).to(dtype) for S in (FLOW["S1"], FLOW["S2"], 1)]


def _module(dtype):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    H, Hkv, Dh = FLOW["H"], FLOW["Hkv"], FLOW["Dh"]
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=Hkv, hidden_size=H * Dh, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=FLOW["L"])
    # the projections are stand-ins: x already is the qkv tensor and the output is returned as it is, so only the attention is under test
    return QuantLlamaAttentionFused(H * Dh, H, FLOW["L"], torch.nn.Identity(), torch.nn.Identity(), DEV, args)


def _composition(xs, dtype, attn, chunk_prefilling=True, decode=True):
    """QuantLlamaAttentionFused.forward's data flow with the kernels the package had before: rope x 2, the torch stores, `attn` on
    natural-layout copies, single_query_attention (tests/test_gpu_attention_prefill.py::test_prompt_then_chunk_then_decode_flow)."""
    E = _engine()
    B, H, Hkv, Dh, L = FLOW["B"], FLOW["H"], FLOW["Hkv"], FLOW["Dh"], FLOW["L"]
    kc = torch.zeros(B, Hkv, Dh // 8, L, 8, dtype=dtype, device=DEV)
    vc = torch.zeros(B, Hkv, L, Dh, dtype=dtype, device=DEV)
    kn = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
    vn = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
    outs, pos = [], 0
    for qkv in xs[:2]:
        S = qkv.shape[1]
        xq, xk, xv = CP.split_qkv(qkv, H, Hkv)
        fr = _freqs(pos, S, Dh)
        xq = E.fused_rope_with_pos_forward_func(xq, fr, True)
        xk = E.fused_rope_with_pos_forward_func(xk, fr, True)
        fill_ft_caches(kc, vc, xk, xv, pos)
        kn[:, pos:pos + S], vn[:, pos:pos + S] = xk, xv
        lo = 0 if chunk_prefilling else pos
        outs.append(attn(xq, kn[:, lo:pos + S], vn[:, lo:pos + S], pos - lo).reshape(B, S, -1))
        pos += S
    if not decode:
        return outs, kc, vc
    xq, xk, xv = CP.split_qkv(xs[2], H, Hkv)
    outs.append(E.single_query_attention(xq[:, 0], xk[:, 0], xv[:, 0], kc, vc, None, None, pos, Dh, 10000.0, 1.0, True).reshape(B, 1, -1))
    return outs, kc, vc


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_prompt_then_chunk_then_decode(dtype):
    xs = _flow_inputs(dtype)
    m = _module(dtype)
    assert m.cache_k.dtype == torch.float16
    ours, pos = [], 0
    for x in xs:
        S = x.shape[1]
        ours.append(m(x, pos, _freqs(pos, S, FLOW["Dh"]) if S > 1 else None, None, chunk_prefilling=pos > 0))
        pos += S
    torch.cuda.synchronize()
    assert m.cache_k.dtype == dtype and m.cache_v.dtype == dtype  # the caches follow the dtype of x on first use
    assert [tuple(o.shape) for o in ours] == [(1, 200, 1024), (1, 56, 1024), (1, 1, 1024)]
    flash = lambda q, k, v, pos: ops.flash_attn_func(q, k, v, None, True)
    want, kc, vc = _composition(xs, dtype, flash)
    for a, b in zip(ours, want):
        assert torch.equal(bits(a), bits(b)), int((bits(a) != bits(b)).sum())
    assert torch.equal(bits(m.cache_k), bits(kc)) and torch.equal(bits(m.cache_v), bits(vc))
    theirs, _, _ = _composition(xs, dtype, eager_attention)
    print("rel per stage:", [round(rel(a, b), 6) for a, b in zip(ours, theirs)])
    for a, b in zip(ours, theirs):
        assert rel(a, b) <= REL[dtype], rel(a, b)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_without_chunk_prefilling_attends_the_new_chunk_only(dtype):
    xs = _flow_inputs(dtype)
    m = _module(dtype)
    ours, pos = [], 0
    for x in xs[:2]:
        S = x.shape[1]
        ours.append(m(x, pos, _freqs(pos, S, FLOW["Dh"]), torch.zeros(1, device=DEV), chunk_prefilling=False))  # (a mask is accepted and ignored)
        pos += S
    flash = lambda q, k, v, pos: ops.flash_attn_func(q, k, v, None, True)
    want, kc, vc = _composition(xs, dtype, flash, chunk_prefilling=False, decode=False)  # (the decode step would add its own k / v)
    for a, b in zip(ours, want):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(m.cache_k), bits(kc)) and torch.equal(bits(m.cache_v), bits(vc))  # the cache is filled all the same
    theirs, _, _ = _composition(xs, dtype, lambda q, k, v, pos: eager_attention(q, k, v, 0), chunk_prefilling=False, decode=False)
    assert rel(ours[1], theirs[1]) <= REL[dtype]
    full, _, _ = _composition(xs, dtype, flash, decode=False)
    assert not torch.equal(bits(ours[1]), bits(full[1]))  # and that differs from attending the history


# ------------------------------------------------------------------------------------------------------------------------
# 5. determinism, graph replay
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128)])
def test_same_call_twice_and_graph_replays_give_the_same_bits(dtype, Dh):
    E = _engine()
    B, H, Hkv, L, pos, S = 2, 8, 2, 400, 230, 90
    g = torch.Generator(device=DEV).manual_seed(11)
    W = (H + 2 * Hkv) * Dh
    data = [torch.randn(B, S, W, generator=g, device=DEV).to(dtype) for _ in range(2)]
    fr = (30.0 * torch.randn(S, B, Dh, generator=g, device=DEV)).contiguous()
    kc = torch.randn(B, Hkv, Dh // 8, L, 8, generator=g, device=DEV).to(dtype)
    vc = torch.randn(B, Hkv, L, Dh, generator=g, device=DEV).to(dtype)
    qkv = data[0].clone()

    def step():
        q = E.rope_kv_store(qkv, fr, kc, vc, pos, H, Hkv)
        return E.attn_prefill_ftcache(q, kc, vc, 0, pos + S, Dh ** -0.5, True)

    want = []
    for d in data:
        qkv.copy_(d)
        a, b = step(), step()
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b))
        want.append(a.clone())
    assert not torch.equal(bits(want[0]), bits(want[1]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        o = step()
    for i in (0, 1, 0):
        qkv.copy_(data[i])  # the inputs are rewritten in place between replays
        kc[:, :, :, pos:pos + S].zero_()
        vc[:, :, pos:pos + S].zero_()
        o.fill_(float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(o), bits(want[i]))
