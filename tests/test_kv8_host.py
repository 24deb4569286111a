"""The FP8 KV cache without a GPU: the numpy restatement of the format (tests/kv8_oracle.py) against torch's float8_e4m3fn, ops.kv8_quant /
ops.kv8_dequant against that restatement bit for bit, the exports and the C ABI's argument checks, the module's constructor, a derived
error bound, and the sharpness of the case lists tests/test_gpu_kv8.py runs: every mutant of the restatement changes their expected
results, and the needle rows hold what they are named for."""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import kv8_oracle as K

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
TORCH_T = {"f16": torch.float16, "bf16": torch.bfloat16}


def t_of(x, dtype):
    """float32 numpy holding T values -> torch tensor of T"""
    return torch.from_numpy(K.to_bits(x, dtype).view(np.int16)).view(TORCH_T[dtype])


def bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------
# the oracle's e4m3fn against torch's
# ------------------------------------------------------------------------------------------------------------------------
def test_oracle_decode_equals_torch_on_every_finite_code():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    finite = (codes & 0x7F) != 0x7F
    assert finite.sum() == 254
    assert np.array_equal(K.DECODE[finite].view(np.uint32), want[finite].view(np.uint32))  # the sign of -0 included
    assert np.isnan(K.DECODE[~finite]).all() and np.isnan(want[~finite]).all()
    assert K.DECODE[0x7E] == 448 and K.DECODE[0x08] == 2.0 ** -6 and K.DECODE[0x01] == 2.0 ** -9


def test_oracle_encode_equals_torch_on_a_dense_sweep_with_every_midpoint():
    pos = K.DECODE[:127].astype(np.float64)
    mids = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), (pos[:-1] + pos[1:]) / 2)  # the midpoints are float32 values
    around = np.concatenate([np.nextafter(mids, np.float32(0)), mids, np.nextafter(mids, np.float32(1000))])
    sub = np.linspace(0, 2.0 ** -6, 4097, dtype=np.float32)                   # the subnormal range, 2^-18 apart
    dense = np.concatenate([np.linspace(0, 448, 200001, dtype=np.float32), np.geomspace(2.0 ** -12, 448, 50001).astype(np.float32)])
    x = np.concatenate([pos.astype(np.float32), around, sub, dense, np.float32([0.0, 448.0])])
    x = np.concatenate([x, -x])
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = K.e4m3_encode(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    # ties go to the even code: the midpoint of codes c and c + 1 encodes to whichever is even
    tie = K.e4m3_encode(mids)
    assert np.array_equal(tie, np.arange(126) + (np.arange(126) % 2))
    assert np.array_equal(K.e4m3_decode(K.e4m3_encode(K.DECODE[:127])), K.DECODE[:127])


# ------------------------------------------------------------------------------------------------------------------------
# ops.kv8_quant / ops.kv8_dequant: the executable statement of the format
# ------------------------------------------------------------------------------------------------------------------------
def _rows(dtype, Dh):
    needles, _ = K.needle_block(dtype, 2, Dh)
    return np.concatenate([needles, K.random_block(dtype, 40, 2, Dh, seed=Dh)])


@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_ops_quant_and_dequant_equal_the_oracle_bit_for_bit(dtype, Dh):
    x = _rows(dtype, Dh)
    codes, scale = K.quant(x)
    tc, ts = ops.kv8_quant(t_of(x, dtype))
    assert tc.dtype == torch.float8_e4m3fn and ts.dtype == torch.float32 and tuple(ts.shape) == x.shape[:-1]
    assert np.array_equal(tc.view(torch.uint8).numpy(), codes)
    assert np.array_equal(ts.numpy().view(np.uint32), scale.view(np.uint32))
    want = K.to_bits(K.dequant(codes, scale, dtype), dtype)
    for c in (tc, tc.view(torch.uint8)):
        back = ops.kv8_dequant(c, ts, TORCH_T[dtype])
        assert back.dtype == TORCH_T[dtype]
        assert np.array_equal(bits_of(back), want)
    assert (scale >= 2.0 ** -60 / 448).all() and (scale[4, 0] == np.float32(2.0 ** -60) / np.float32(448))  # the zero row: the floor, no denormal
    with pytest.raises(TypeError):
        ops.kv8_quant(torch.zeros(2, 64))
    with pytest.raises(ValueError):
        ops.kv8_dequant(tc, ts[:1], TORCH_T[dtype])


@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_roundtrip_error_is_inside_the_derived_bound(dtype, Dh):
    """|dequant(quant(x)) - x| <= max(2^-4 |x|, 2^-10 s) + ulp_T(|x|), every element.  y = x / s lies in [-448, 448] up to one fp32
    rounding; the nearest e4m3 value is within half a spacing, 2^-4 |y| for a normal result (3 mantissa bits) and 2^-10 for a subnormal
    one (spacing 2^-9) -- times s.  The fp32 division and multiply add 2^-24 relative each and the rounding to T half an ulp of the
    result, which lies within (1 + 2^-4) of x: together below one ulp_T(|x|)."""
    x = _rows(dtype, Dh)
    codes, scale = K.quant(x)
    back = K.dequant(codes, scale, dtype).astype(np.float64)
    xd = x.astype(np.float64)
    lim = np.maximum(2.0 ** -4 * np.abs(xd), 2.0 ** -10 * scale.astype(np.float64)[..., None]) + K.ulp(xd, dtype)
    err = np.abs(back - xd)
    assert (err <= lim).all(), float((err / lim).max())
    assert (err > 0).any()


# ------------------------------------------------------------------------------------------------------------------------
# exports, signatures, argument checks (no GPU call)
# ------------------------------------------------------------------------------------------------------------------------
def test_library_engine_and_ops_export_the_kv8_surface():
    L = _capi.lib()
    for name in ("awq_rope_kv_store_natural_fp8", "awq_attn_prefill_kv8", "awq_attn_splitkv_kv8"):
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
    assert L.awq_abi_version() == 1
    assert len(_capi.SIGNATURES["awq_rope_kv_store_natural_fp8"][1]) == 20
    assert len(_capi.SIGNATURES["awq_attn_prefill_kv8"][1]) == 26 and len(_capi.SIGNATURES["awq_attn_splitkv_kv8"][1]) == 28
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params(eng.rope_kv_store_natural_fp8) == ["qkv", "freqs", "k_cache", "v_cache", "k_scale", "v_scale", "start_pos", "nheads", "nheads_kv"]
    assert params(eng.attn_prefill_kv8) == params(eng.attn_splitkv_kv8) == ["q", "k", "v", "k_scale", "v_scale", "softmax_scale", "causal"]
    assert list(inspect.signature(ops.rope_kv_store_natural_fp8).parameters) == params(eng.rope_kv_store_natural_fp8)
    for name in ("attn_prefill_kv8", "attn_splitkv_kv8", "attn_kv8"):
        assert list(inspect.signature(getattr(ops, name)).parameters) == ["q", "k", "v", "k_scale", "v_scale", "softmax_scale", "causal"]
    assert list(inspect.signature(ops.kv8_quant).parameters) == ["x"]
    assert list(inspect.signature(ops.kv8_dequant).parameters) == ["codes", "scale", "dtype"]
    assert list(inspect.signature(ops.flash_attn_func).parameters) == ["q", "k", "v", "softmax_scale", "causal"]  # untouched


def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _attn(entry, p, **kw):
    # Sk = 4096, Sq * G = 4: the plan splits, so a valid split call needs a workspace -- which stays NULL: nothing is ever launched
    a = dict(q=p, k=p, v=p, ks=p, vs=p, out=p, B=1, Sq=1, Sk=4096, H=8, Hkv=2, Dh=128, qbs=1024, qrs=1024, kbs=4096 * 256, krs=256,
             vbs=4096 * 256, vrs=256, ksbs=4096 * 2, ksrs=2, vsbs=4096 * 2, vsrs=2, scale=0.1, causal=1, dtype=0, ws=None, wsb=0)
    a.update(kw)
    head = (a["q"], a["k"], a["v"], a["ks"], a["vs"], a["out"], a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"], a["kbs"],
            a["krs"], a["vbs"], a["vrs"], a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"], a["scale"], a["causal"], a["dtype"])
    if entry == "prefill":
        return _capi.lib().awq_attn_prefill_kv8(*head, None)
    return _capi.lib().awq_attn_splitkv_kv8(*head, a["ws"], a["wsb"], None)


@pytest.mark.parametrize("entry", ["prefill", "splitkv"])
def test_kv8_attention_argument_validation_returns_codes_without_launch(entry):
    buf, p = _p16()
    for bad in (dict(Dh=96), dict(Dh=72, causal=0), dict(Dh=32), dict(H=6, Hkv=4), dict(Sq=4097), dict(B=0), dict(Sq=0), dict(Sk=0), dict(Hkv=0),
                dict(qrs=512), dict(krs=128), dict(vrs=240), dict(ksrs=1), dict(vsrs=0), dict(qbs=-8), dict(ksbs=-2)):
        assert _attn(entry, p, **bad) == AWQ_ERR_SHAPE, bad
    assert _attn(entry, p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "ks", "vs", "out"):
        assert _attn(entry, p, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):                      # a misaligned cache: 16 bytes
        assert _attn(entry, p, **{name: p + 8}) == AWQ_ERR_ALIGN, name
    for name in ("ks", "vs"):                                # a misaligned scale: 4 bytes (and 4 is enough)
        assert _attn(entry, p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    for name, val in (("krs", 264), ("vrs", 264), ("kbs", 4096 * 256 + 8), ("vbs", 4096 * 256 + 8), ("qrs", 1028), ("qbs", 1028)):
        assert _attn(entry, p, **{name: val}) == AWQ_ERR_ALIGN, name  # code strides: multiples of 16
    if entry == "splitkv":
        need = _capi.lib().awq_attn_splitkv_workspace_bytes(1, 8, 2, 128, 1, 4096, 1)
        assert need == 8 * ops.attn_splitkv_plan(1, 8, 2, 128, 1, 4096, True)[0] * 130 * 4 > 0  # the T cache's formula
        assert _attn(entry, p) == AWQ_ERR_WORKSPACE
        assert _attn(entry, p, ks=p + 4, vs=p + 4) == AWQ_ERR_WORKSPACE  # 4-byte aligned scales pass the checks
        assert _attn(entry, p, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE
        assert _attn(entry, p, ws=None, wsb=need) == AWQ_ERR_WORKSPACE
        assert _attn(entry, p, ws=p + 4, wsb=need) == AWQ_ERR_ALIGN


def test_kv8_store_argument_validation_returns_codes_without_launch():
    buf, p = _p16()
    f = _capi.lib().awq_rope_kv_store_natural_fp8
    ok = dict(qkv=p, fr=p, q=p, kc=p, vc=p, ks=p, vs=p, B=1, Bc=2, S=4, H=8, Hkv=2, Dh=128, rot=128, lmax=64, start=3, bs=4 * 1536, rs=1536,
              dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], a["ks"], a["vs"], a["B"], a["Bc"], a["S"], a["H"], a["Hkv"], a["Dh"], a["rot"],
                 a["lmax"], a["start"], a["bs"], a["rs"], a["dtype"], None)
    for bad in (dict(Dh=96), dict(Dh=72), dict(rot=24), dict(rot=144), dict(rot=0), dict(B=3), dict(B=0), dict(S=0), dict(H=0), dict(Hkv=0),
                dict(start=-1), dict(start=61), dict(lmax=0), dict(rs=1528), dict(bs=-8)):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    assert call(dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "fr", "q", "kc", "vc", "ks", "vs"):
        assert call(**{name: None}) == AWQ_ERR_NULL, name
    for name in ("qkv", "fr", "q", "kc", "vc"):
        assert call(**{name: p + 4}) == AWQ_ERR_ALIGN, name
    for name in ("ks", "vs"):
        assert call(**{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert call(bs=4 * 1536 + 4) == AWQ_ERR_ALIGN and call(rs=1540) == AWQ_ERR_ALIGN


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    q = torch.zeros(1, 1, 8, 128, dtype=torch.float16)
    k = torch.zeros(1, 64, 2, 128, dtype=torch.float8_e4m3fn)
    s = torch.zeros(1, 64, 2)
    for fn in (ops.attn_kv8, ops.attn_prefill_kv8, ops.attn_splitkv_kv8):
        with pytest.raises(_capi.AwqNativeError, match="GPU"):
            fn(q, k, k, s, s, causal=True)


# ------------------------------------------------------------------------------------------------------------------------
# the module's constructor
# ------------------------------------------------------------------------------------------------------------------------
def _module(**kw):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    H, Hkv, Dh = 4, 2, 64
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=Hkv, hidden_size=H * Dh, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=96)
    return QuantLlamaAttentionFused(H * Dh, H, 96, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3, **kw)


def test_module_constructor_owns_the_fp8_buffers_and_refuses_the_rest():
    m = _module(kv_layout="natural", kv_dtype="fp8")
    assert m.kv_dtype == "fp8" and m.kv_layout == "natural"
    for c in (m.cache_k, m.cache_v):
        assert tuple(c.shape) == (3, 96, 2, 64) and c.dtype == torch.float8_e4m3fn and c.is_contiguous()
    for s in (m.cache_k_scale, m.cache_v_scale):
        assert tuple(s.shape) == (3, 96, 2) and s.dtype == torch.float32 and s.is_contiguous()
    with pytest.raises(ValueError, match="kv_layout"):
        _module(kv_layout="ft", kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_layout"):
        _module(kv_dtype="fp8")  # the default layout is "ft"
    for bad in ("int8", "e5m2", "fp16", ""):
        with pytest.raises(ValueError, match="kv_dtype"):
            _module(kv_layout="natural", kv_dtype=bad)
    for kw in (dict(kv_layout="natural"), dict(kv_layout="natural", kv_dtype=None), dict()):
        m = _module(**kw)
        assert m.kv_dtype is None and m.cache_k.dtype == torch.float16
        assert not hasattr(m, "cache_k_scale") and not hasattr(m, "cache_v_scale")
    from llm_awq_amd.fused_attn import make_quant_attn
    assert list(inspect.signature(make_quant_attn).parameters) == ["model", "dev", "max_batch_size", "kv_layout", "kv_dtype"]


# ------------------------------------------------------------------------------------------------------------------------
# sharpness: the needle rows hold what they are named for, and every mutant changes the case lists' expected results
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_needle_rows_hold_their_conditions(dtype, Dh):
    rows, names = K.needle_block(dtype, 2, Dh)
    assert np.array_equal(K.round_to(rows, dtype), rows) and np.isfinite(rows).all()
    row = dict(zip(names, rows))
    amax = lambda t: np.abs(t).max(axis=-1)
    a = amax(row["heads-2^10-apart"])
    assert 2.0 ** 8 < a[1] / a[0] < 2.0 ** 12
    t = row["amax-last-column"]
    assert (np.abs(t).argmax(axis=-1) == Dh - 1).all() and (amax(t[:, :Dh // 2]) < amax(t) / 16).all()
    t = row["midpoints"][0]
    s = amax(t) / np.float32(448)
    y = (t[:Dh - 1][t[:Dh - 1] != 0] / s).astype(np.float64)
    assert len(y) >= 63
    pos = K.DECODE[:127].astype(np.float64)
    mids = (pos[:-1] + pos[1:]) / 2
    assert np.isin(np.abs(y), mids).all() and (np.abs(y) < 2.0 ** -6).any() and (np.abs(y) > 1).any() and (y < 0).any()  # subnormal and normal range
    t = row["divide"][0]
    s = amax(t) / np.float32(448)
    n = int((t[:Dh - 1] != 0).sum())
    assert n >= 4 and (K.e4m3_encode(np.clip(t[:n] / s, -448, 448)) != K.e4m3_encode(np.clip(t[:n] * (np.float32(1) / s), -448, 448))).all()
    t = row["zero-row"]
    assert not t[0].any() and not np.signbit(t[0]).any() and np.signbit(t[1]).all() and not t[1].any()
    if dtype == "f16":
        t = row["f16-60000"][0]
        assert t.max() == 60000 and t.min() == -60000
        c, s = K.quant(row["f16-60000"])
        assert np.isfinite(K.dequant(c, s, dtype)).all() and c[0, 1] == 0x7E and c[0, Dh - 2] == 0xFE
    else:
        assert "f16-60000" not in row


def _changed(a, b):
    return any(not np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_changes_the_store_cases_expected_results(mutant):
    """The store test compares codes and scales (and the attention tests what the staging makes of them) with the oracle's; of a store
    case's K only the tokens the rotation leaves alone are known here, V whole."""
    seen = 0
    for case in K.STORE_CASES:
        qkv, freqs, plain, k, v = K.store_inputs(case)
        assert plain.any() and not freqs[plain.T].any()
        kk = k[plain]  # [tokens, Hkv, Dh]
        vv = v.reshape(-1, *v.shape[2:])
        good = K.cache_roundtrip(kk, vv[:len(kk)], case["dtype"]) + K.cache_roundtrip(vv, vv, case["dtype"])[2:]
        bad = K.cache_roundtrip(kk, vv[:len(kk)], case["dtype"], mutant) + K.cache_roundtrip(vv, vv, case["dtype"], mutant)[2:]
        seen += _changed(good, bad)
    # one token holds one needle: a case of S = 1 need not meet the needle a mutant shows at, the cases of S >= 5 do
    assert seen >= sum(c["S"] >= 5 for c in K.STORE_CASES), (mutant, seen)


@pytest.mark.parametrize("mutant", ["per_token", "k_scale_on_v"])
def test_scale_indexing_mutants_change_every_attention_case(mutant):
    shapes = {(c["Sq"], c["Sk"], c["G"], c["Dh"], c["dtype"]) for c in K.SPLIT_FORCED + K.SPLIT_PLAN}
    shapes |= {(Sq, Sk, G, c["Dh"], c["dtype"]) for c in K.ONEPASS for (Sq, Sk, _) in K.ONEPASS_SHAPES for G in (1, 4)}
    for Sq, Sk, G, Dh, dtype in sorted(shapes):
        if Sk > 300 and Dh == 128:
            continue  # (the same generator at another head dim: one head dim of the long cases is enough here)
        d = K.attn_inputs(Sq, Sk, G, Dh, dtype)
        good = K.cache_roundtrip(d["k"], d["v"], dtype)
        assert np.array_equal(good[0], d["kc"][:, :Sk]) and np.array_equal(good[3].view(np.uint32), d["vs"][:, :Sk].view(np.uint32))
        assert (d["kc"][:, Sk:] == 0x7F).all() and np.isnan(d["ks"][:, Sk:]).all() and np.isnan(d["vs"][:, Sk:]).all()
        assert _changed(good[4:], K.cache_roundtrip(d["k"], d["v"], dtype, mutant)[4:]), (Sq, Sk, G, Dh, dtype)
        ratio = d["ks"][:, :Sk].max() / d["ks"][:, :Sk].min()
        assert Sk < 32 or ratio >= 2.0 ** 8  # the per-key scales are spread


def test_case_lists_cover_the_axes_of_the_issue():
    assert {(c["S"], c["Dh"], c["dtype"], c["start"]) for c in K.STORE_CASES} == {(S, Dh, dt, st) for S in (1, 5, 67) for Dh in (64, 128)
                                                                                  for dt in K.DTYPES for st in (0, 61)}
    assert (K.STORE["B"], K.STORE["Bc"], K.STORE["H"], K.STORE["Hkv"], K.STORE["lmax"]) == (2, 3, 4, 2, 160)
    assert len(K.SPLIT_FORCED) == 3 * 2 * 2 * 2 * 2 * 2 and K.CHUNK == 64
    assert {(c["Sq"], c["Sk"]) for c in K.SPLIT_PLAN} == {(1, 2049), (4, 2111)} and (K.ATTN_B, K.ATTN_HKV) == (2, 2)
    assert set(K.ONEPASS_TILES) == {64, 128, 256}
    assert {(Sq, Sk) for Sq, Sk, c in K.ONEPASS_SHAPES if c} == {(Sq, Sk) for Sq in (1, 33, 130) for Sk in (1, 63, 65, 193) if Sq <= Sk}
    assert {(Sq, Sk) for Sq, Sk, c in K.ONEPASS_SHAPES if not c} == {(Sq, Sk) for Sq in (1, 33, 130) for Sk in (1, 63, 65, 193)}
