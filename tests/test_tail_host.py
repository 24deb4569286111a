"""CPU: the references of tests/tail_oracle.py behave on their own, and they are sharp -- numpy restatements of plausible kernel faults are each
REJECTED by the inputs and acceptance sets tests/test_gpu_tails.py uses.  Every mutant states how many of those inputs it fails on (its reach, for the
default AWQ_TEST_SEED) and the test asserts the reach is above zero: a mutant that fails nowhere would prove nothing about the check."""
import numpy as np
import pytest
import torch

from tests import tail_oracle as TO
from tests.helpers import SEED0, rmsnorm_uncertainty

DTYPES = [torch.bfloat16, torch.float16]
_memo = {}


def _sweep(dtype):
    """the standalone sweep of test_gpu_tails: all gates x the 64 ups, with its acceptance set"""
    if ("sweep", dtype) not in _memo:
        _memo["sweep", dtype] = TO.sweep_accept(dtype, TO.up_values(dtype))
    return _memo["sweep", dtype]


def _ordered(bits):
    b = bits.astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


# ---------------- conditions on the reference ----------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_hull_is_at_most_one_code_wide_and_rarely_ambiguous(dtype):
    g = TO.all_patterns(dtype)
    lo, hi = TO.silu_hull(g)
    x = g.double().numpy()
    fin = np.isfinite(x)
    lb, hb = TO.to_bits(lo), TO.to_bits(hi)
    dist = np.abs(_ordered(lb) - _ordered(hb))
    nan = np.isnan(x) | (np.isinf(x) & (x < 0))
    assert (dist[~nan] <= 1).all(), "lo and hi more than one code apart"
    assert torch.isnan(lo.float())[torch.from_numpy(nan)].all() and torch.isnan(hi.float())[torch.from_numpy(nan)].all()
    assert not torch.isnan(lo.float())[torch.from_numpy(~nan)].any()
    amb = int(((lb != hb) & fin).sum())
    print(f"{dtype}: {amb} of {int(fin.sum())} finite gates with lo != hi")
    assert amb <= 0.005 * fin.sum(), amb
    # the pinned specials: +-0 -> +-0 (bits), +inf -> +inf
    for v in (0.0, -0.0, float("inf")):
        t = torch.tensor([v], dtype=torch.float64).to(dtype)
        l1, h1 = TO.silu_hull(t)
        assert TO.to_bits(l1)[0] == TO.to_bits(t)[0] == TO.to_bits(h1)[0]
    # the tighter delta never exceeds the plain (4 + |x|) 2^-23
    assert (TO.silu_delta(x[fin]) <= (4.0 + np.abs(x[fin])) * 2.0 ** -23).all()


def test_band_counts():
    """the gate classes no statistical test reaches are in the sweep"""
    for dtype in DTYPES:
        g = TO.all_patterns(dtype)
        x = g.double().numpy()
        fin = np.isfinite(x)
        e_T = TO.rne64_to_T(TO.silu64(np.where(fin, x, 0.0)), dtype).double().numpy()
        deep = int((fin & (x < -64) & (e_T != 0)).sum())
        sub = int((fin & (e_T != 0) & (np.abs(e_T) < TO.smallest_normal(dtype))).sum())
        if dtype == torch.bfloat16:
            assert deep == 66, deep
        else:
            assert sub >= 100, sub
        assert int((TO.to_bits(g) == 0).sum()) == 1 and int((TO.to_bits(g) == 0x8000).sum()) == 1
        eg = TO.edge_gates(dtype)
        ex = eg.double().numpy()
        assert (TO.to_bits(eg) == 0).any() and (TO.to_bits(eg) == 0x8000).any()
        assert ((ex < TO.SILU_MIN_AT).any() and (ex > TO.SILU_MIN_AT).any() and np.isfinite(ex).all())
        if dtype == torch.bfloat16:
            assert int(((ex < -64) & (TO.rne64_to_T(TO.silu64(ex), dtype).double().numpy() != 0)).sum()) == 66


@pytest.mark.parametrize("dtype", DTYPES)
def test_rne_to_T_equals_torch_cpu_conversion(dtype):
    p = TO.rounding_patterns(dtype)
    assert p.numel() % 8 == 0
    got, want = TO.rne_to_T(p, dtype), p.to(dtype)
    assert bool((torch.isnan(got) == torch.isnan(want)).all())
    ok = TO.bits_equal_or_nan(got, want)
    assert bool(ok.all()), (int((~ok).sum()), p[~ok][:4], got[~ok][:4], want[~ok][:4])
    assert int(torch.isnan(want).sum()) >= 4 and int(torch.isinf(want).sum()) >= 4
    sub = (want.double().abs() > 0) & (want.double().abs() < TO.smallest_normal(dtype))
    assert int(sub.sum()) > 100, "subnormal results must be in the pattern set"


@pytest.mark.parametrize("dtype", DTYPES)
def test_rne64_to_T_agrees_with_rne_to_T_on_fp32_values(dtype):
    """the two roundings of this module state the same function where both apply (fp32 inputs)"""
    p = TO.rounding_patterns(dtype)
    a = TO.rne64_to_T(p.double().numpy(), dtype)
    assert bool(TO.bits_equal_or_nan(a, TO.rne_to_T(p, dtype)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_evaluation_is_accepted(dtype):
    """a correctly rounded fp32 silu, rounded to T, times up, rounded to T -- passes the acceptance set everywhere it is pinned"""
    gate, up, c_lo, c_hi, pinned = _sweep(dtype)
    s32 = torch.from_numpy(TO.silu64(gate.double().numpy()).astype(np.float32))
    sT = TO.rne_to_T(s32, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        out = TO.rne64_to_T(sT.double().numpy() * up.double().numpy(), dtype)
    bad, _l, _h = TO.tail_check(out, c_lo, c_hi)
    assert not bool((bad & pinned).any()), int((bad & pinned).sum())


# ---------------- mutants: SiLU * mul ----------------
def _silu32_model(x32: np.ndarray, rescue: bool) -> np.ndarray:
    """the kernel's formula in numpy fp32 with the hardware's flush: rcp returns 0 where its result would be an fp32 subnormal"""
    x32 = x32.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        k = np.where(x32 < -64, np.float32(2.0 ** -64), np.float32(1.0)) if rescue else np.float32(1.0)
        den = (np.float32(1.0) + np.exp2(x32 * np.float32(-1.4426950408889634), dtype=np.float32)) * k
        r = (np.float32(1.0) / den).astype(np.float32)
        r = np.where(np.abs(r) < np.float32(2.0 ** -126), np.float32(0.0), r)
        return (x32 * r * k).astype(np.float32)


def _mut_no_rescue(dtype):
    gate, up, c_lo, c_hi, pinned = _sweep(dtype)
    col = 0  # up = 1
    g = gate[:, col]
    sT = TO.rne_to_T(torch.from_numpy(_silu32_model(g.float().numpy(), rescue=False)), dtype)
    bad, _l, _h = TO.tail_check(sT, c_lo[:, col], c_hi[:, col])  # (T(s * 1) = s)
    return bad & pinned[:, col] & ~torch.isnan(g)


def _mut_single_rounding(dtype):
    gate, up, c_lo, c_hi, pinned = _sweep(dtype)
    s32 = TO.silu64(gate.double().numpy()).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = TO.rne64_to_T(s32 * up.double().numpy(), dtype)
    bad, _l, _h = TO.tail_check(out, c_lo, c_hi)
    return bad & pinned


def _selector_setup(dtype):
    key = ("sel", dtype)
    if key not in _memo:
        K, F = 512, 256
        g, u = TO.edge_pairs(dtype)
        x = TO.selector_x(g, u, K)
        gg, uu = TO.selector_pairs(x, F)
        _memo[key] = (x, F, TO.tail_accept(gg, uu))
    return _memo[key]


def _mut_swapped_deinterleave(dtype):
    x, F, (c_lo, c_hi) = _selector_setup(dtype)
    gs, us = TO.selector_pairs(x, F, swapped=True)
    lo, _hi = TO.tail_accept(gs, us)
    bad, _l, _h = TO.tail_check(lo, c_lo, c_hi)
    return bad


def _second_trip(dtype):
    """the second-trip call: gate patterns cycling, up = 1 + ulp; -> (pattern index int64 [n], per-pattern c_lo, c_hi, pinned)"""
    key = ("trip", dtype)
    if key not in _memo:
        g = TO.all_patterns(dtype)
        up = TO.rne64_to_T(np.full(65536, 1.0 + TO.one_ulp(dtype)), dtype)
        c_lo, c_hi = TO.tail_accept(g, up)
        pinned = ~(torch.isinf(g.float()) & (g.float() < 0))
        _memo[key] = (torch.arange(TO.SILU_SECOND_TRIP) % 65536, c_lo, c_hi, pinned)
    return _memo[key]


def _mut_silu_first_trip_only(dtype):
    idx, c_lo, c_hi, pinned = _second_trip(dtype)
    out = c_lo[idx].clone()
    out[TO.SILU_FIRST_TRIP:] = float("nan")  # the poison a skipped store leaves
    bad, _l, _h = TO.tail_check(out, c_lo[idx], c_hi[idx])
    return bad & pinned[idx]


# ---------------- mutants: fp32 -> T (+ bias) ----------------
def _trunc_to_T(f32, dtype):
    u = f32.contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    if dtype == torch.bfloat16:
        return TO.from_bits((u >> 16).astype(np.uint16), dtype)
    # fp16: drop the bits below the result's last place (round toward zero), through the exact-value route
    v = f32.double().numpy()
    a = np.abs(np.where(np.isfinite(v), v, 1.0))
    _m, ex = np.frexp(a)
    q = np.exp2(np.maximum(ex - 1, TO.MIN_EXP[dtype]).astype(np.float64) - TO.MANT[dtype])
    r = np.minimum(np.floor(a / q) * q, TO.T_MAX[dtype])
    r = np.where(np.isfinite(v), np.copysign(r, v), v)
    return torch.from_numpy(r).to(dtype)


def _mut_truncation(dtype):
    p = TO.rounding_patterns(dtype)
    return ~TO.bits_equal_or_nan(_trunc_to_T(p, dtype), TO.rne_to_T(p, dtype))


def _mut_add_7fff_no_nan_guard(dtype):
    assert dtype == torch.bfloat16
    p = TO.rounding_patterns(dtype)
    u = p.view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    h = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return ~TO.bits_equal_or_nan(TO.from_bits(h.astype(np.uint16), dtype), TO.rne_to_T(p, dtype))


def _flush32(t: torch.Tensor) -> torch.Tensor:
    return torch.where(t.abs() < 2.0 ** -126, torch.copysign(torch.zeros_like(t), t), t)


def _mut_flush_input(dtype):
    assert dtype == torch.bfloat16
    p = TO.rounding_patterns(dtype)
    return ~TO.bits_equal_or_nan(TO.rne_to_T(_flush32(p), dtype), TO.rne_to_T(p, dtype))


def _bias_case(dtype, m=300, n=264):
    key = ("bias", dtype, m, n)
    if key not in _memo:
        y, b = TO.round_inputs(dtype, m, n), TO.bias_values(dtype, n)
        _memo[key] = (y, b, TO.round_bias_ref(y, b, dtype))
    return _memo[key]


def _mut_flush_output(dtype):
    assert dtype == torch.bfloat16
    y, b, want = _bias_case(dtype)
    s = _flush32(TO.rne_to_T(y, dtype).float() + b.float()[None, :])
    return ~TO.bits_equal_or_nan(TO.rne_to_T(s, dtype), want)


def _mut_bias_before_rounding(dtype):
    y, b, want = _bias_case(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        got = TO.rne64_to_T(y.double().numpy() + b.double().numpy()[None, :], dtype)
    return ~TO.bits_equal_or_nan(got, want)


def _mut_bias_one_octet_off(dtype):
    out = None
    for (m, n) in ((300, 264), (4, 8)):
        y, b, want = _bias_case(dtype, m, n)
        got = TO.round_bias_ref(y, torch.roll(b, -8), dtype)  # bias[(col + 8) % n]
        bad = ~TO.bits_equal_or_nan(got, want)
        if n == 8:
            assert not bool(bad.any()), "a bias of one octet has period 8: the offset cannot show there"
        else:
            out = bad
    return out


def _mut_round_first_trip_only(dtype):
    m, n = TO.ROUND_BIG
    y, b, want = _bias_case(dtype, m, n)
    got = want.clone()
    got.reshape(-1)[TO.ROUND_FIRST_TRIP:] = float("nan")
    return ~TO.bits_equal_or_nan(got, want)


# ---------------- mutants: RMSNorm ----------------
def _mut_rmsnorm_one_wave(dtype):
    """rstd from part[0] alone: wave 0 holds the 16-byte granules gi with gi % 256 < 64"""
    bad_all = []
    for K in TO.RMS_K:
        x, gamma = TO.rmsnorm_rows(K, dtype)
        ref = TO.rmsnorm_ref(x, gamma, TO.RMS_EPS)
        unc = rmsnorm_uncertainty(x, gamma, TO.RMS_EPS)
        wave0 = ((torch.arange(K) // 8) % 256) < 64
        xd = x.double()
        got = TO.rmsnorm_ref(x, gamma, TO.RMS_EPS, tot=(xd * xd)[:, wave0].sum(-1, keepdim=True))
        bad = (got.double() - ref.double()).abs() > unc
        if K <= 512:
            assert not bool(bad.any()), "up to 512 columns wave 0 holds the whole row"
        bad_all.append(bad.reshape(-1))
    return torch.cat(bad_all)


MUTANTS = [
    # (name, function, dtype, reach at AWQ_TEST_SEED = 0)
    ("silu without the < -64 rescue", _mut_no_rescue, torch.bfloat16, 20),
    ("silu not rounded to T before the multiply", _mut_single_rounding, torch.bfloat16, 61916),
    ("silu not rounded to T before the multiply", _mut_single_rounding, torch.float16, 472842),
    ("selector gate / up swapped", _mut_swapped_deinterleave, torch.bfloat16, 5645),
    ("selector gate / up swapped", _mut_swapped_deinterleave, torch.float16, 16285),
    ("silu * mul grid-stride loop stops after one trip", _mut_silu_first_trip_only, torch.bfloat16, 2056),
    ("silu * mul grid-stride loop stops after one trip", _mut_silu_first_trip_only, torch.float16, 2056),
    ("truncation instead of RNE", _mut_truncation, torch.bfloat16, 98160),
    ("truncation instead of RNE", _mut_truncation, torch.float16, 95238),
    ("bf16 add-0x7FFF without a NaN guard", _mut_add_7fff_no_nan_guard, torch.bfloat16, 4),
    ("fp32 denormals flushed on input", _mut_flush_input, torch.bfloat16, 1270),
    ("fp32 denormals flushed on output", _mut_flush_output, torch.bfloat16, 12),
    ("bias added in fp32 before the one rounding", _mut_bias_before_rounding, torch.bfloat16, 2691),
    ("bias added in fp32 before the one rounding", _mut_bias_before_rounding, torch.float16, 13365),
    ("bias index off by one octet", _mut_bias_one_octet_off, torch.bfloat16, 59257),
    ("bias index off by one octet", _mut_bias_one_octet_off, torch.float16, 75073),
    ("round_bias grid-stride loop stops after one trip", _mut_round_first_trip_only, torch.bfloat16, 49216),
    ("round_bias grid-stride loop stops after one trip", _mut_round_first_trip_only, torch.float16, 49216),
    ("rmsnorm reads part[] of one wave only", _mut_rmsnorm_one_wave, torch.bfloat16, 79851),
    ("rmsnorm reads part[] of one wave only", _mut_rmsnorm_one_wave, torch.float16, 79847),
]


@pytest.mark.parametrize("name,fn,dtype,reach", MUTANTS, ids=[f"{m[0]} [{str(m[2]).split('.')[-1]}] reach={m[3]}" for m in MUTANTS])
def test_mutant_is_rejected(name, fn, dtype, reach):
    bad = fn(dtype)
    n = int(bad.sum())
    print(f"{name} [{dtype}]: rejected on {n} of {bad.numel()} inputs")
    assert n > 0, f"mutant '{name}' passes the check: the check proves nothing about this fault"
    if SEED0 == 0:
        assert n == reach, f"mutant '{name}': reach {n}, stated {reach}"
