"""Decode attention without a GPU: the C ABI's argument checks and host plan, the drop-in exports of awq_inference_engine, and
self-checks of the float64 oracle (tests/attn_oracle.py)."""
import ctypes

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_oracle as A

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7


def test_engine_exports_reference_signatures():
    eng = llm_awq_amd.load_engine()
    assert hasattr(eng, "single_query_attention") and hasattr(eng, "layernorm_forward_cuda")
    doc = eng.single_query_attention.__doc__.splitlines()[0]
    # keyword names, order and defaults of the reference binding (pybind.cpp:25-28)
    names = ["q", "k", "v", "k_cache", "v_cache", "length_per_sample_", "alibi_slopes_", "timestep", "rotary_embedding_dim",
             "rotary_base", "rotary_scale", "neox_rotary_style"]
    params = [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params == names, doc
    for key, default in (("rotary_embedding_dim", "0"), ("rotary_base", "10000.0"), ("rotary_scale", "1.0"), ("neox_rotary_style", "True")):
        seg = doc[doc.index(key + ":"):]
        assert seg.split(",")[0].split(")")[0].endswith(f"= {default}"), (key, doc)
    assert eng.layernorm_forward_cuda.__doc__.startswith("layernorm_forward_cuda(")


def _bufs():
    buf = (ctypes.c_char * 8192)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    return buf, p16


def _call(p16, **kw):
    a = dict(q=p16, k=p16, v=p16, kc=p16, vc=p16, lens=None, alibi=None, out=p16, B=1, Bc=1, H=8, Hkv=2, Dh=128, L=64,
             qbs=1024, kbs=256, vbs=256, t=5, rot=0, base=10000.0, scale=1.0, neox=1, dtype=0, ws=None, wsb=0)
    a.update(kw)
    return _capi.lib().awq_attn_decode(a["q"], a["k"], a["v"], a["kc"], a["vc"], a["lens"], a["alibi"], a["out"], a["B"], a["Bc"],
                                       a["H"], a["Hkv"], a["Dh"], a["L"], a["qbs"], a["kbs"], a["vbs"], a["t"], a["rot"], a["base"],
                                       a["scale"], a["neox"], a["dtype"], a["ws"], a["wsb"], None)


def test_argument_validation_returns_codes_without_launch():
    buf, p = _bufs()
    for bad in (dict(Dh=24), dict(Dh=48 + 8), dict(Dh=272), dict(H=6, Hkv=4), dict(B=2, Bc=1), dict(rot=3), dict(rot=130),
                dict(t=-1), dict(L=0), dict(B=0), dict(Hkv=0), dict(rot=-2)):
        assert _call(p, **bad) == AWQ_ERR_SHAPE, bad
    assert _call(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "kc", "vc", "out"):
        assert _call(p, **{name: None}) == AWQ_ERR_NULL, name
        assert _call(p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _call(p, qbs=1028) == AWQ_ERR_ALIGN
    assert _call(p, lens=p + 2) == AWQ_ERR_ALIGN
    assert _call(p, alibi=p + 1) == AWQ_ERR_ALIGN
    # a plan with splits needs the workspace
    L = _capi.lib()
    need = L.awq_attn_decode_workspace_bytes(1, 8, 2, 128, 8191, 8192)
    assert need > 0
    assert _call(p, t=8191, L=8192) == AWQ_ERR_WORKSPACE
    assert _call(p, t=8191, L=8192, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE
    s, c = ctypes.c_int(), ctypes.c_int()
    assert L.awq_attn_decode_plan(1, 8, 100, 10, 64, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_decode_plan(1, 8, 128, -1, 64, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_decode_plan(1, 8, 128, 10, 64, None, ctypes.byref(c)) == AWQ_ERR_NULL


MODELS = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128), "qwen2_7b": (28, 4, 128), "llama3_70b_tp8": (8, 1, 128)}
# (splits, chunk) per (model, B, L) with timestep = L - 1 and Lmax = L
PINNED = {
    ("llama3_8b", 1, 1): (1, 256), ("llama3_8b", 1, 128): (1, 256), ("llama3_8b", 1, 4096): (16, 256), ("llama3_8b", 1, 32768): (32, 1024),
    ("llama3_8b", 8, 1): (1, 256), ("llama3_8b", 8, 128): (1, 256), ("llama3_8b", 8, 4096): (4, 1024), ("llama3_8b", 8, 32768): (4, 8192),
    ("llama2_7b", 1, 1): (1, 256), ("llama2_7b", 1, 128): (1, 256), ("llama2_7b", 1, 4096): (8, 512), ("llama2_7b", 1, 32768): (8, 4096),
    ("llama2_7b", 8, 1): (1, 256), ("llama2_7b", 8, 128): (1, 256), ("llama2_7b", 8, 4096): (1, 4096), ("llama2_7b", 8, 32768): (1, 32768),
    ("qwen2_7b", 1, 1): (1, 256), ("qwen2_7b", 1, 128): (1, 256), ("qwen2_7b", 1, 4096): (16, 256), ("qwen2_7b", 1, 32768): (64, 512),
    ("qwen2_7b", 8, 1): (1, 256), ("qwen2_7b", 8, 128): (1, 256), ("qwen2_7b", 8, 4096): (8, 512), ("qwen2_7b", 8, 32768): (8, 4096),
    ("llama3_70b_tp8", 1, 1): (1, 256), ("llama3_70b_tp8", 1, 128): (1, 256), ("llama3_70b_tp8", 1, 4096): (16, 256),
    ("llama3_70b_tp8", 1, 32768): (128, 256),
    ("llama3_70b_tp8", 8, 1): (1, 256), ("llama3_70b_tp8", 8, 128): (1, 256), ("llama3_70b_tp8", 8, 4096): (16, 256),
    ("llama3_70b_tp8", 8, 32768): (32, 1024),
}


@pytest.mark.parametrize("key", sorted(PINNED))
def test_plan_is_pinned_and_workspace_agrees(key):
    model, B, L = key
    H, Hkv, Dh = MODELS[model]
    splits, chunk = ops.attn_decode_plan(B, Hkv, Dh, L - 1, L)
    assert (splits, chunk) == PINNED[key]
    assert chunk % 256 == 0 and (splits - 1) * chunk < L <= splits * chunk or splits == 1
    if B * Hkv >= 256 or L <= 256:
        assert splits == 1
    else:
        assert B * Hkv * splits >= 256 or chunk == 256  # fills the chip, or every split is one tile
    wsb = _capi.lib().awq_attn_decode_workspace_bytes(B, H, Hkv, Dh, L - 1, L)
    assert wsb == (0 if splits == 1 else B * H * splits * (Dh + 4) * 4)


def test_plan_depends_on_host_arguments_only_and_caps_at_lmax():
    assert ops.attn_decode_plan(1, 8, 128, 100000, 4096) == ops.attn_decode_plan(1, 8, 128, 4095, 4096)
    assert ops.attn_decode_plan(1, 1, 128, 8191, 8192) == (32, 256)  # 70B TP=8 at 8 k: the split alone gives 32 blocks


def test_oracle_without_rotary_is_a_row_of_causal_attention():
    g = torch.Generator().manual_seed(0)
    T, Dh, L = 40, 64, 64
    Q, K, V = (torch.randn(T, Dh, generator=g, dtype=torch.float64).to(torch.float32) for _ in range(3))
    full = A.causal_attention(Q, K, V)
    kc = A.to_ft_k_cache(K.reshape(1, 1, T, Dh).repeat(1, 1, 2, 1)[:, :, :L])
    vc = V.reshape(1, 1, T, Dh).repeat(1, 1, 2, 1)[:, :, :L].contiguous()
    for t in (0, 1, 17, T - 1):
        out, k_rot, _ = A.decode(Q[t].reshape(1, 1, Dh), K[t].reshape(1, 1, Dh), V[t].reshape(1, 1, Dh), kc, vc, timestep=t)
        torch.testing.assert_close(out[0, 0], full[t], rtol=1e-5, atol=1e-6)  # (only the 1e-6 of the FT denominator differs)
        assert torch.equal(k_rot[0, 0], K[t])


def test_oracle_neox_rotary_is_rotate_half():
    g = torch.Generator().manual_seed(1)
    for Dh, rot, base, scale, t in ((128, 128, 10000.0, 1.0, 77), (64, 32, 500000.0, 0.25, 4095)):
        x = torch.randn(3, Dh, generator=g, dtype=torch.float64)
        got = A.rotate(x, t, rot, base, scale, True, emulate_fp32=False)
        inv = 1.0 / base ** (torch.arange(0, rot, 2, dtype=torch.float64) / rot)
        f = torch.cat([t * scale * inv] * 2)
        xr = x[:, :rot]
        half = torch.cat([-xr[:, rot // 2:], xr[:, :rot // 2]], -1)
        want = torch.cat([xr * f.cos() + half * f.sin(), x[:, rot:]], -1)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_oracle_rotary_is_identity_at_position_zero():
    x = torch.randn(4, 96).to(torch.bfloat16)
    for neox in (True, False):
        for rot in (32, 96):
            assert torch.equal(A.rotate(x, 0, rot, 10000.0, 1.0, neox), x)
