"""The needle / pair cases of tests/attn_cases.py without a GPU: for every parameter set that tests/test_gpu_attention_needle.py
runs (the same list object), the conditions that make the GPU test's bit comparison meaningful.

  * every target element is exact in T, nonzero and normal;
  * the float64 oracle alone, rounded to T, returns the target bits, and lies within 2^-16 (relative, per element) of the target:
    the smallest half-ulp is 2^-12 (fp16) / 2^-9 (bf16) relative, which leaves the kernel's fp32 arithmetic a factor of 16 and
    more (exp(0) is exact; one division, one reduction);
  * the needles lie in [first_step, t] and really sit on the first and last position of every split, either side of the claimed
    256-tile edges and on the wrap pair of a circular cache (the host plan is used to aim, never as an expected value);
  * oracle-level faults (a dropped position, the stale cache slot, KV head + 1, batch row + 1, first_step off by one either way, a
    wrong rotary style / dim / base / scale) each break the bit comparison wherever the construction is bound to see them.
"""
import numpy as np
import pytest
import torch

from llm_awq_amd import ops
from tests import attn_cases as C
from tests import attn_oracle as A

REL_ORACLE = 2.0 ** -16


def _bits_equal(out64: torch.Tensor, target: torch.Tensor) -> bool:
    return torch.equal(out64.to(target.dtype).view(torch.int16), target.view(torch.int16))


def _check_target(tg: torch.Tensor, exact32: np.ndarray):
    fi = torch.finfo(tg.dtype)
    assert torch.equal(tg.float(), torch.from_numpy(exact32)), "target not exact in T"
    assert (tg.float().abs() >= fi.tiny).all() and torch.isfinite(tg.float()).all(), "target zero / subnormal / non-finite"


def _claimed_edges(case):
    """(row, position) pairs that the case must hold a needle on, computed here from the plan and the launch code's split rule."""
    s = case.spec
    splits, chunk = ops.attn_decode_plan(s["B"], s["Hkv"], s["Dh"], s["t"], s["Lmax"])
    mode = s.get("positions", "edges")
    need = []
    for b in range(s["B"]):
        tl = case.T[b]
        first = max(0, tl + 1 - s["Lmax"])
        assert first == case.first[b]
        edges = []
        for j in range(splits):
            lo = first + j * chunk
            hi = tl + 1 if j == splits - 1 else min(tl + 1, lo + chunk)
            if hi <= lo:
                continue
            need += [(b, lo), (b, hi - 1)]
            edges += list(range(lo + 256, hi, 256))
        if edges:
            pick = edges if mode in ("all_edges", "exhaust") else [edges[0], edges[len(edges) // 2], edges[-1]]
            for e in pick:
                need += [(b, e - 1), (b, e)]
        need += [(b, first), (b, min(first + 1, tl)), (b, max(tl - 1, first)), (b, tl)]
        if tl >= s["Lmax"]:
            # (t % Lmax == Lmax - 1: the walk starts in slot 0 and never wraps)
            for w in (p for p in range(first, tl) if p % s["Lmax"] == s["Lmax"] - 1):
                need += [(b, w), (b, w + 1)]
    return need, splits, chunk


@pytest.mark.parametrize("spec", C.CASES, ids=C.case_id)
def test_case_conditions(spec):
    case = C.Case(spec)
    s, dt = case.spec, case.dtype
    B, H, Dh = s["B"], s["H"], s["Dh"]
    salt_h = np.repeat(case.salt, case.G, axis=1)
    # needles in range; split / tile / wrap edges hit
    for b in range(B):
        assert (case.needles[:, b] >= case.first[b]).all() and (case.needles[:, b] <= case.T[b]).all()
    if case.kind == "needle":
        need, splits, chunk = _claimed_edges(case)
        if case.lens is None:
            have = set(case.needles.reshape(-1).tolist())
            missing = [p for _, p in need if p not in have]
        else:
            have = [set(case.needles[:, b].reshape(-1).tolist()) for b in range(B)]
            missing = [(b, p) for b, p in need if p not in have[b]]
        assert not missing, missing[:10]
        if s.get("positions") == "exhaust":  # every attended position exactly once
            flat = np.sort(case.needles.reshape(-1))
            assert np.array_equal(flat, np.arange(case.first[0], s["t"] + 1))
        elif case.lens is None and case.T[0] - case.first[0] + 1 >= B * H:
            for c in range(case.ncalls):  # every query head of a call has a needle of its own
                assert len(set(case.needles[c].reshape(-1).tolist())) == B * H
    if s["group"] == "onesplit" or s["name"].startswith(("stair-onesplit", "mirror-onesplit")):
        assert B * s["Hkv"] >= 256 and case.splits == 1 and s["t"] >= 4095
    if case.kind in ("stair", "mirror"):
        # the decoy in the first tile and the needle in the last one (or mirrored): the running maximum moves between tiles
        lo_hi = [r for r in C.split_ranges(case.first[0], s["t"], case.splits, case.chunk) if r[1] > r[0]]
        first_tile_end = lo_hi[0][0] + 256
        last_tile = lo_hi[-1][0] + ((lo_hi[-1][1] - 1 - lo_hi[-1][0]) // 256) * 256
        nd, dc = case.needles[0][:, ::case.G], case.decoy
        lo, hi = (dc, nd) if case.kind == "stair" else (nd, dc)
        assert (lo < first_tile_end).all() and (hi >= last_tile).all()
    # the oracle alone returns the target, to the bit and within 2^-16
    out0 = None
    for c in range(case.ncalls):
        tg = case.target(c)
        exact = C.vrow(case.needles[c], salt_h, Dh, case.fixed_sign)
        if case.kind == "pair":
            exact = (exact + C.vrow(np.full_like(case.needles[c], s["pair"][1]), salt_h, Dh, True)) / 2
        _check_target(tg, exact)
        out, _, _ = A.decode(case.q(c), case.k, case.v, case.kc, case.vc, case.lens, case.alibi, s["t"], case.rot, case.base,
                             case.scale, case.neox)
        assert torch.isfinite(out).all()
        assert _bits_equal(out, tg), (c, (out.to(dt).view(torch.int16) != tg.view(torch.int16)).nonzero()[:4])
        rel = ((out - tg.double()).abs() / tg.double().abs()).max().item()
        assert rel <= REL_ORACLE, (c, rel)
        if c == 0:
            out0 = out
    # the builders' own fault sensitivity
    assert torch.equal(C.decode_mut(case, 0, None), out0)  # the restated oracle is the oracle
    tg0 = case.target(0)
    ran = 0
    for m in C.MUTANTS:
        if C.mutant_applies(case, m):
            assert not _bits_equal(C.decode_mut(case, 0, m), tg0), f"mutant {m} passes the bit comparison"
            ran += 1
    assert ran >= 3


def test_every_requested_axis_is_in_the_list():
    names = [s["name"] for s in C.CASES]
    assert len(set(names)) == len(names)
    for dt in (torch.float16, torch.bfloat16):
        cs = [s for s in C.CASES if s["dtype"] == dt]
        grp = [s for s in cs if s["group"] == "groups"]
        assert {s["H"] // s["Hkv"] for s in grp} >= {1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 32}
        assert {s["Hkv"] for s in grp} >= {1, 2, 8, 32}
        assert any(s["Hkv"] == 1 and s["H"] == 32 for s in grp) and any(s["Hkv"] == 32 and s["H"] == 32 for s in grp)
        assert {s["Dh"] for s in cs} >= set(range(32, 257, 16))
        for Dh in (32, 80, 128, 256):
            assert any(s["Dh"] == Dh and ops.attn_decode_plan(s["B"], s["Hkv"], Dh, s["t"], s["Lmax"])[0] > 1 for s in grp)
        rot = {(s["rot"], s["base"], s["scale"], s["t"], s["Dh"]) for s in cs if s["group"] == "rotary"}
        assert len(rot) == 4 * 2 * 4 * 2
        assert any(s["Lmax"] & (s["Lmax"] - 1) and s["t"] >= s["Lmax"] for s in cs)  # a circular cache that is no power of two


def test_alibi_too_steep_for_an_exact_needle_is_refused():
    with pytest.raises(ValueError):
        C.Case(dict(name="x", group="alibi", dtype=torch.float16, B=1, H=2, Hkv=1, Dh=32, Lmax=32768, t=32767, alibi=True))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_large_cache_construction_at_a_small_size(dtype):
    p = C.LARGE_SMALL
    q, k, v, kc, vc, t, needles, target = C.build_large("cpu", dtype, **p)
    G, Hkv, B = p["G"], p["Hkv"], p["B"]
    assert t in needles.tolist() and 0 in needles.tolist()
    _check_target(target, C.vrow(needles, np.full_like(needles, C.LARGE_SALT), p["Dh"], False))
    out, _, _ = A.decode(q, k, v, kc, vc, None, None, t)
    assert torch.isfinite(out).all()
    mine = out[B - 1, (Hkv - 1) * G:]
    assert _bits_equal(mine, target)
    assert ((mine - target.double()).abs() / target.double().abs()).max().item() <= REL_ORACLE
    # the stale slot, and the needles read from another batch row or KV head, break it
    k2, v2 = k.clone(), v.clone()
    k2[B - 1, Hkv - 1] = A.k_cache_rows(kc, B - 1, Hkv - 1, [t % p["Lmax"]])[0]
    v2[B - 1, Hkv - 1] = vc[B - 1, Hkv - 1, t % p["Lmax"]]
    assert not _bits_equal(A.decode(q, k2, v2, kc, vc, None, None, t)[0][B - 1, (Hkv - 1) * G:], target)
    for roll_dim in (0, 1):
        o = A.decode(q, k, v, torch.roll(kc, 1, roll_dim), torch.roll(vc, 1, roll_dim), None, None, t)[0]
        assert not _bits_equal(o[B - 1, (Hkv - 1) * G:], target)
