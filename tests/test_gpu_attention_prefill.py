"""Prefill attention on the MI355X (csrc/awq_attn_prefill_cdna4.hip): the needle cases of tests/attn_prefill_cases.py bit for bit,
random inputs against the float64 oracle (tests/attn_prefill_oracle.py) under a derived elementwise bound, determinism and graph
replay, agreement with the decode kernel, the reference's eager attention as a second opinion, and the prompt-then-decode flow of
tinychat's QuantLlamaAttentionFused restated here (tinychat/modules/fused_attn.py; the reference tree is not read by GPU tests)."""
import math

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from tests import attn_oracle as A
from tests import attn_prefill_cases as C
from tests import attn_prefill_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _flash():
    llm_awq_amd.install_as_flash_attn()
    from flash_attn import flash_attn_func  # the module name tinychat imports (llama.py:21, fused_attn.py:17)

    return flash_attn_func


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


# ------------------------------------------------------------------------------------------------------------------------
# 7. needle cases: bit equality, every row, both entry points
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_needle_cases_bit_exact(spec):
    case = C.Case(spec)
    q, k, v = case.to(DEV)
    assert q.stride() == case.q.stride() and k.stride() == case.k.stride()
    want = case.target.view(torch.int16)
    out = ops.flash_attn_func(q, k, v, case.scale, case.causal)
    torch.cuda.synchronize()
    assert out.shape == case.target.shape and out.is_contiguous()
    got = out.cpu().view(torch.int16)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())
    out2 = _flash()(q, k, v, 0.0, case.scale, case.causal)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu().view(torch.int16), want)


# ------------------------------------------------------------------------------------------------------------------------
# 8. random inputs against float64, elementwise
# ------------------------------------------------------------------------------------------------------------------------
def make(B, H, Hkv, Dh, Sq, Sk, dtype, seed, fused=False):
    """The distributions of tests/test_gpu_attention.py::make (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N), drawn on the GPU."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dtype)
    k = torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV).to(dtype)
    v = (1 + 0.5 * torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV)).to(dtype)
    if fused:
        S = max(Sq, Sk) + 2
        qkv = torch.full((B, S, (H + 2 * Hkv) * Dh), float("nan"), dtype=dtype, device=DEV)
        qkv[:, :Sq, :H * Dh] = q.reshape(B, Sq, -1)
        qkv[:, :Sk, H * Dh:(H + Hkv) * Dh] = k.reshape(B, Sk, -1)
        qkv[:, :Sk, (H + Hkv) * Dh:] = v.reshape(B, Sk, -1)
        q = qkv[:, :Sq, :H * Dh].view(B, Sq, H, Dh)
        k = qkv[:, :Sk, H * Dh:(H + Hkv) * Dh].view(B, Sk, Hkv, Dh)
        v = qkv[:, :Sk, (H + Hkv) * Dh:].view(B, Sk, Hkv, Dh)
    return q, k, v


def check_bound(out, q, k, v, scale, causal, dtype):
    Dh, Sk = q.shape[-1], k.shape[1]
    sc = Dh ** -0.5 if scale is None else scale
    ref, Aw, qk = O.attention(q, k, v, scale, causal, stats=True)
    lim = O.bound(ref, Aw, qk, dtype, Sk, Dh, sc)
    err = (out.double() - ref).abs()
    assert torch.isfinite(out.float()).all()
    print(f"max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())
    return ref


def _random_cases():
    out = []
    squares = (1, 2, 63, 64, 65, 127, 129, 1000, 4096)
    chunks = ((1, 500), (130, 700), (512, 2560), (96, 1500))
    groups, batches = (1, 4, 7, 8), (1, 3)
    n = 0
    for Sq, Sk in [(s, s) for s in squares] + list(chunks):
        for j, dt in enumerate((torch.float16, torch.bfloat16)):
            # every axis has its own period and the dtype offsets each of them, so that over the 13 shapes both dtypes meet every
            # group size, both batches, both head dims and both KV head counts
            m = n + j
            G, B, Dh, Hkv = groups[(m + j) % 4], batches[(m // 2 + j) % 2], (64, 128)[(m // 3) % 2], (2, 1)[(m // 5 + j) % 2]
            if Sq >= 4096:
                B = 1
            out.append(dict(dtype=dt, B=B, G=G, Hkv=Hkv, Dh=Dh, Sq=Sq, Sk=Sk, causal=True, fused=((n + j) % 3 == 0)))
        n += 1
    out.append(dict(dtype=torch.bfloat16, B=2, G=4, Hkv=2, Dh=128, Sq=100, Sk=333, causal=False, fused=False))
    out.append(dict(dtype=torch.float16, B=1, G=1, Hkv=3, Dh=64, Sq=333, Sk=100, causal=False, fused=True))
    out.append(dict(dtype=torch.bfloat16, B=1, G=4, Hkv=1, Dh=128, Sq=8192, Sk=8192, causal=True, fused=False))  # S = 8192 once
    out.append(dict(dtype=torch.float16, B=4, G=4, Hkv=8, Dh=128, Sq=600, Sk=600, causal=True, fused=True))      # 128-row q tiles
    out.append(dict(dtype=torch.bfloat16, B=8, G=4, Hkv=8, Dh=128, Sq=1100, Sk=1100, causal=True, fused=False))  # 256-row q tiles
    out.append(dict(dtype=torch.float16, B=1, G=8, Hkv=8, Dh=64, Sq=300, Sk=300, causal=True, fused=False))      # 64-row q tiles
    return out


@pytest.mark.parametrize("c", _random_cases(), ids=lambda c: f"{str(c['dtype'])[6:]}-B{c['B']}-G{c['G']}-Hkv{c['Hkv']}-Dh{c['Dh']}-{c['Sq']}x{c['Sk']}"
                         + ("" if c["causal"] else "-full") + ("-fused" if c["fused"] else ""))
def test_random_inputs_within_the_derived_bound(c):
    H = c["G"] * c["Hkv"]
    q, k, v = make(c["B"], H, c["Hkv"], c["Dh"], c["Sq"], c["Sk"], c["dtype"], seed=c["Sq"] * 31 + c["Sk"] + c["Dh"], fused=c["fused"])
    out = ops.flash_attn_func(q, k, v, None, c["causal"])
    check_bound(out, q, k, v, None, c["causal"], c["dtype"])
    out2 = _flash()(q, k, v, causal=c["causal"])
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_softmax_scale_argument(dtype):
    q, k, v = make(2, 8, 2, 128, 130, 700, dtype, seed=5)
    out = ops.flash_attn_func(q, k, v, 0.05, True)
    check_bound(out, q, k, v, 0.05, True, dtype)


# ------------------------------------------------------------------------------------------------------------------------
# 9. determinism, graph capture
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128)])
def test_same_call_twice_and_graph_replays_give_the_same_bits(dtype, Dh):
    q, k, v = make(2, 16, 4, Dh, 700, 900, dtype, seed=11, fused=True)
    f = _flash()
    a = f(q, k, v, causal=True)
    b = f(q, k, v, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f(q, k, v, causal=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        o = f(q, k, v, causal=True)
    for _ in range(3):
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), a.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------
# torch restatements of what tinychat does around the attention call
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


def fill_ft_caches(kc, vc, k, v, start_pos):
    """fused_attn.py:259-267: v_cache [B, Hkv, L, Dh] <- v, k_cache [B, Hkv, Dh/8, L, 8] <- k at positions start_pos .. start_pos + S."""
    B, S, Hkv, Dh = k.shape
    vc[:B, :, start_pos:start_pos + S, :] = v.transpose(1, 2)
    kc[:B, :, :, start_pos:start_pos + S, :] = k.reshape(B, S, Hkv, Dh // 8, 8).permute(0, 2, 3, 1, 4)


def rotate_neox(x, start_pos, base=10000.0):
    """Rotate-half rotary embedding of x [B, S, heads, Dh] at positions start_pos .. start_pos + S - 1, in fp32, rounded to T."""
    Dh = x.shape[-1]
    inv = 1.0 / (base ** (torch.arange(0, Dh, 2, device=x.device).float() / Dh))
    ang = torch.outer(torch.arange(start_pos, start_pos + x.shape[1], device=x.device).float(), inv)[None, :, None, :]
    a, b = x.float()[..., :Dh // 2], x.float()[..., Dh // 2:]
    return torch.cat([a * ang.cos() - b * ang.sin(), b * ang.cos() + a * ang.sin()], -1).to(x.dtype)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ------------------------------------------------------------------------------------------------------------------------
# 11. the reference's eager path as a second opinion
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Sq,Sk,G,Dh", [(300, 300, 4, 128), (130, 700, 1, 64), (1, 500, 8, 128), (1000, 1000, 7, 64)])
def test_eager_composition_agrees(dtype, Sq, Sk, G, Dh):
    q, k, v = make(2, 2 * G, 2, Dh, Sq, Sk, dtype, seed=Sq + Sk + G)
    out = _flash()(q, k, v, causal=True)
    ref = eager_attention(q, k, v, Sk - Sq)
    assert rel(out, ref) <= REL[dtype], rel(out, ref)


# ------------------------------------------------------------------------------------------------------------------------
# 10. prefill and decode agree
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("S,G,Dh", [(65, 4, 128), (700, 1, 64), (1000, 8, 128)])
def test_prefill_and_decode_agree_on_the_last_row(dtype, S, G, Dh):
    B, Hkv = 2, 2
    H = G * Hkv
    q, k, v = make(B, H, Hkv, Dh, S, S, dtype, seed=S + G)
    q, k = rotate_neox(q, 0), rotate_neox(k, 0)  # rotary applied in torch, as llama.py's prefill does; the decode side then takes rotary_embedding_dim = 0
    out = ops.flash_attn_func(q, k, v, None, True)
    ref, Aw, qk = O.attention(q[:, S - 1:], k, v, None, True, stats=True)
    lim_prefill = O.bound(ref, Aw, qk, dtype, S, Dh, Dh ** -0.5)
    assert not ((out[:, S - 1:].double() - ref).abs() > lim_prefill).any()
    # the decode step of token S - 1 over a cache of S - 1 entries, no rotary
    L = S + 7
    kc = torch.full((B, Hkv, Dh // 8, L, 8), float("nan"), dtype=dtype, device=DEV)
    vc = torch.full((B, Hkv, L, Dh), float("nan"), dtype=dtype, device=DEV)
    fill_ft_caches(kc, vc, k[:, :S - 1], v[:, :S - 1], 0)
    dec = ops.single_query_attention(q[:, S - 1].contiguous(), k[:, S - 1].contiguous(), v[:, S - 1].contiguous(), kc, vc, None, None,
                                     timestep=S - 1, rotary_embedding_dim=0)
    # decode: 1 ulp of T (tests/test_gpu_attention.py) plus FT's 1e-6 in the denominator: |o| * 1e-6 / sum_j p_j, sum_j p_j >= 1
    lim = lim_prefill[:, 0] + A.ulp(ref[:, 0], dtype) + 1e-6 * ref[:, 0].abs()
    err = (dec.double() - out[:, S - 1].double()).abs()
    assert not (err > lim).any(), float((err / lim).max())


# ------------------------------------------------------------------------------------------------------------------------
# 13. prompt, second chunk, one decode step: QuantLlamaAttentionFused.forward's data flow
# ------------------------------------------------------------------------------------------------------------------------
def _freqs(start, n, Dh, base=10000.0):
    inv = 1.0 / (base ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    t = torch.arange(start, start + n, device=DEV).float()
    f = torch.outer(t, inv)
    return torch.cat([f, f], -1)[None].contiguous()  # [1, n, Dh]: one angle per column, rotate-half layout


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_prompt_then_chunk_then_decode_flow(dtype):
    """The q / k / v slices of the qkv tensor follow the distributions of make() (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N), for which REL is
    meant: the eager side rounds its scores to T (2^-4 at |s| ~ 10 in bf16), an error of its own that only averages out over a v with
    a common component; on a zero-mean v it alone exceeds REL."""
    E, flash = _engine(), _flash()
    B, H, Hkv, Dh, L = 1, 8, 2, 128, 512
    S1, S2 = 200, 56
    mul = torch.cat([torch.full((H * Dh,), 1.5), torch.ones(Hkv * Dh), torch.full((Hkv * Dh,), 0.5)]).to(DEV)
    add = torch.cat([torch.zeros((H + Hkv) * Dh), torch.ones(Hkv * Dh)]).to(DEV)

    def run(attn):
        kc = torch.zeros(B, Hkv, Dh // 8, L, 8, dtype=dtype, device=DEV)
        vc = torch.zeros(B, Hkv, L, Dh, dtype=dtype, device=DEV)
        kn = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)  # the natural-layout copies the eager path reads
        vn = torch.zeros(B, L, Hkv, Dh, dtype=dtype, device=DEV)
        outs, pos = [], 0
        gg = torch.Generator(device=DEV).manual_seed(3)
        for S in (S1, S2):
            qkv = (torch.randn(B, S, (H + 2 * Hkv) * Dh, generator=gg, device=DEV) * mul + add).to(dtype)
            xq = qkv[:, :, :H * Dh].view(B, S, H, Dh)
            xk = qkv[:, :, H * Dh:(H + Hkv) * Dh].view(B, S, Hkv, Dh)
            xv = qkv[:, :, (H + Hkv) * Dh:].view(B, S, Hkv, Dh)
            fr = _freqs(pos, S, Dh)
            xq = E.fused_rope_with_pos_forward_func(xq, fr, True)
            xk = E.fused_rope_with_pos_forward_func(xk, fr, True)
            fill_ft_caches(kc, vc, xk, xv, pos)
            kn[:, pos:pos + S], vn[:, pos:pos + S] = xk, xv
            outs.append(attn(xq, kn[:, :pos + S], vn[:, :pos + S], pos))
            pos += S
        qkv = (torch.randn(B, (H + 2 * Hkv) * Dh, generator=gg, device=DEV) * mul + add).to(dtype)
        xq, xk, xv = qkv[:, :H * Dh].view(B, H, Dh), qkv[:, H * Dh:(H + Hkv) * Dh].view(B, Hkv, Dh), qkv[:, (H + Hkv) * Dh:].view(B, Hkv, Dh)
        outs.append(E.single_query_attention(xq, xk, xv, kc, vc, None, None, pos, Dh, 10000.0, 1.0, True))
        return outs

    ours = run(lambda q, k, v, pos: flash(q, k, v, causal=True))
    theirs = run(lambda q, k, v, pos: eager_attention(q, k, v, pos))
    assert ours[0].shape == (B, S1, H, Dh) and ours[1].shape == (B, S2, H, Dh)
    print("rel per stage:", [round(rel(a, b), 6) for a, b in zip(ours, theirs)])
    for a, b in zip(ours, theirs):
        assert rel(a, b) <= REL[dtype], rel(a, b)
