"""Needle and pair cases for decode attention: inputs whose exact answer is known to the bit.

A *needle* case builds K so that, for query head h, one attended position p*(h) scores at least GAP_MIN above every other
position; the softmax weight outside it is then below N * exp(-GAP_MIN) and the output of head h must be the bit pattern of the
V row of p*(h).  A *pair* case gives two positions bit-identical key rows, so their weights are exactly equal and the output is
the bit pattern of (V[p1] + V[p2]) / 2.  A *stair* case adds a decoy one gap below the needle (and removes every other row that
close), so the running maximum of a block that walks the context rises more than once.

    key of position p        code(p + salt)[d] = -1 if bit (d % 16) of (p + salt) else +1;  salt depends on (batch row, KV head)
    query                    q[h] = amp * code(p*(h) + salt), amp = 32 (raised with ALiBi until the gap condition holds)
    gap                      one flipped bit flips Dh / 16 dims: amp * 2 * (Dh / 16) / sqrt(Dh) >= 22.6 at amp = 32
    value row                V[p][d] = sign * (1 + ((p + 3 d + 2 salt) % 64) / 64): 6 fraction bits (7 for the mean of two), exact in
                             fp16 and bf16, never zero; sign = code(p + salt)[d] (the signs spell p), or a fixed pattern in d for
                             pair cases (so that the mean of two rows cannot cancel).  The magnitudes take 2 * salt: the row that
                             another (batch row, KV head) keeps under the same code then still differs
    current token            through k / v; its cache slot, every slot outside [first_step, t] and every cache row >= B hold NaN
    rotary                   the cache rows hold the code rotated at the *current* position t in float64 and rounded to T (q is
                             rotated at t only and a rotation keeps dot products); k holds the un-rotated code of position t

CASES is the one list of parameter sets: tests/test_attention_needle_host.py proves on the CPU, for every entry, that the float64
oracle alone returns the target bits (and that oracle-level faults do not), tests/test_gpu_attention_needle.py runs the same
entries through the kernel.  The host plan (awq_attn_decode_plan, no GPU needed) is used to aim needles at split and tile edges,
never as an expected value.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from llm_awq_amd import ops
from tests import attn_oracle as A

TILE = 256
GAP_MIN = 22.0   # N * exp(-22) <= 2^15 * 2.8e-10 < 2^-16: the oracle stays within 2^-16 of the target row
AMP = 32.0
ROTS = ("none", "half_neox", "full_neox", "half_gptj", "full_gptj")
MUTANTS = ("drop", "stale", "kvh+1", "row+1", "first-1", "first+1", "rot_style", "rot_dim", "rot_base", "rot_scale")


def rot_of(name: str, Dh: int):
    if name == "none":
        return 0, True
    return (Dh if name.startswith("full") else Dh // 2), name.endswith("neox")


def code(x, Dh: int) -> np.ndarray:
    """x: int array [...] -> float32 [..., Dh] of +-1."""
    x = np.asarray(x, dtype=np.int64)
    bits = (x[..., None] >> (np.arange(Dh) % 16)) & 1
    return (1 - 2 * bits).astype(np.float32)


def pair_sign(Dh: int) -> np.ndarray:
    return np.where(np.arange(Dh) % 3 == 0, -1.0, 1.0).astype(np.float32)


def vrow(p, salt, Dh: int, fixed_sign: bool) -> np.ndarray:
    """Value rows of positions p (int array [...], salt broadcastable to it) -> float32 [..., Dh]."""
    p = np.asarray(p, dtype=np.int64)
    salt = np.asarray(salt, dtype=np.int64)
    mag = 1.0 + ((p[..., None] + 3 * np.arange(Dh) + 2 * salt[..., None]) % 64) / 64.0
    sgn = pair_sign(Dh) if fixed_sign else code(p + salt, Dh)
    return (sgn * mag).astype(np.float32)


def salt_of(b: int, kvh: int, Hkv: int, tmax: int) -> int:
    return (13 + 7919 * (b * Hkv + kvh)) % (65535 - tmax)


def split_ranges(first: int, tl: int, splits: int, chunk: int):
    """[begin, end) of every split of a row at length tl, as the launch code states it (empty splits included)."""
    out = []
    for j in range(splits):
        lo = first + j * chunk
        hi = tl + 1 if j == splits - 1 else min(tl + 1, lo + chunk)
        out.append((lo, max(lo, hi)))
    return out


def tile_edges(first: int, tl: int, splits: int, chunk: int):
    """Positions e such that e - 1 and e lie in the same split but in different 256-tiles of its walk."""
    return [e for lo, hi in split_ranges(first, tl, splits, chunk) for e in range(lo + TILE, hi, TILE)]


def edge_positions(first: int, tl: int, splits: int, chunk: int, Lmax: int, all_tiles: bool = False):
    want = [first, first + 1, tl - 1, tl]
    for lo, hi in split_ranges(first, tl, splits, chunk):
        if hi > lo:
            want += [lo, hi - 1]
    te = tile_edges(first, tl, splits, chunk)
    if te:
        for e in (te if all_tiles else (te[0], te[len(te) // 2], te[-1])):
            want += [e - 1, e]
    if tl >= Lmax:  # circular: the position in slot Lmax - 1 and its successor in slot 0
        w = (first // Lmax) * Lmax + Lmax - 1
        if w < first:
            w += Lmax
        want += [w, w + 1]
    seen, out = set(), []
    for p in want:
        if first <= p <= tl and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _fill(edges, first: int, tl: int, count: int):
    """edges, then distinct scattered positions of [first, tl] until `count` entries (or the range is used up)."""
    n = tl - first + 1
    out, seen = list(edges), set(edges)
    i = 0
    while len(out) < min(count, n):
        p = first + (i * 2654435761 + 977) % n
        i += 1
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


class Case:
    """One built parameter set: CPU tensors q(call) / k / v / kc / vc (FT layouts), lens, alibi, kw and the targets."""

    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        B, H, Hkv, Dh, Lmax, t = s["B"], s["H"], s["Hkv"], s["Dh"], s["Lmax"], s["t"]
        self.Bc = Bc = s.get("Bc") or B
        self.G = G = H // Hkv
        self.kind = kind = s.get("kind", "needle")
        self.rot, self.neox = rot_of(s.get("rot", "none"), Dh)
        self.base, self.scale = s.get("base", 10000.0), s.get("scale", 1.0)
        self.splits, self.chunk = ops.attn_decode_plan(B, Hkv, Dh, t, Lmax)
        lens = s.get("lens")
        if lens is not None:
            sym = {"zero": 0, "small": min(300, self.chunk - 1), "edge-1": self.chunk - 1, "edge": self.chunk, "max": t,
                   "edge2": 2 * self.chunk, "mid": t // 2 + 1}
            lens = [sym[x] if isinstance(x, str) else int(x) for x in lens]
            assert len(lens) == B and max(lens) <= t
        self.T = T = lens if lens is not None else [t] * B
        self.lens = torch.tensor(lens, dtype=torch.int32) if lens is not None else None
        self.first = first = [max(0, tl + 1 - Lmax) for tl in T]
        self.salt = np.array([[salt_of(b, kvh, Hkv, max(T)) for kvh in range(Hkv)] for b in range(B)], dtype=np.int64)
        assert int(self.salt.max()) + max(T) < 65536  # distinct codes over the attended positions
        if B * Hkv <= 64:
            assert len(set(self.salt.reshape(-1).tolist())) == B * Hkv
        fixed_sign = self.fixed_sign = kind == "pair"

        # ---- needle table [ncalls, B, H] ----
        mode = s.get("positions", "edges")
        rows = []
        for b in range(B):
            if mode == "exhaust":
                rows.append(list(range(first[b], T[b] + 1)))
            else:
                rows.append(edge_positions(first[b], T[b], self.splits, self.chunk, Lmax, all_tiles=(mode == "all_edges")))
        self.claimed = rows  # the positions this case claims to aim at (before the filling)
        if kind == "needle":
            if lens is None:
                P = _fill(rows[0], first[0], t, -(-len(rows[0]) // (B * H)) * (B * H))
                self.ncalls = max(1, -(-len(rows[0]) // (B * H)))
                idx = (np.arange(self.ncalls * B * H) % len(P)).reshape(self.ncalls, B, H)
                self.needles = np.asarray(P, dtype=np.int64)[idx]
            else:
                self.ncalls = max(1, max(-(-len(r) // H) for r in rows))
                self.needles = np.zeros((self.ncalls, B, H), dtype=np.int64)
                for b in range(B):
                    P = _fill(rows[b], first[b], T[b], -(-len(rows[b]) // H) * H)
                    self.needles[:, b, :] = np.asarray(P, dtype=np.int64)[(np.arange(self.ncalls * H) + s.get("shift", 0)) % len(P)].reshape(self.ncalls, H)
        elif kind == "pair":
            p1, p2 = s["pair"]
            assert lens is None and self.rot == 0 and first[0] <= p1 < p2 <= t
            self.ncalls = 1
            self.needles = np.full((1, B, H), p1, dtype=np.int64)
        else:  # stair / mirror: one needle per (b, KV head), shared by its query heads
            assert lens is None and self.rot == 0 and kind in ("stair", "mirror")
            self.ncalls = 1
            self.needles = np.zeros((1, B, H), dtype=np.int64)
            self.decoy = np.zeros((B, Hkv), dtype=np.int64)
            last_lo = [r for r in split_ranges(first[0], t, self.splits, self.chunk) if r[1] > r[0]][-1]
            last_tile = last_lo[0] + ((last_lo[1] - 1 - last_lo[0]) // TILE) * TILE
            for b in range(B):
                for kvh in range(Hkv):
                    i = b * Hkv + kvh
                    hi_p = max(last_tile, t - 1 - i % 200)
                    lo_p = first[0] + 5 + i % 200
                    needle, decoy = (hi_p, lo_p) if kind == "stair" else (lo_p, hi_p)
                    self.needles[0, b, kvh * G:(kvh + 1) * G] = needle
                    self.decoy[b, kvh] = decoy
        for b in range(B):
            assert (self.needles[:, b] >= first[b]).all() and (self.needles[:, b] <= T[b]).all()

        # ---- amplitude: with ALiBi the needle's score falls by slope * (t - p*) against a position at t ----
        self.alibi = None
        self.amp = AMP
        unit_gap = 2.0 * (Dh // 16) / math.sqrt(Dh)
        if s.get("alibi"):
            self.alibi = (0.01 + 0.05 * (torch.arange(H, dtype=torch.float32) + 1) / H)
            worst = float(self.alibi.max()) * max(T[b] - first[b] for b in range(B))
            while self.amp * unit_gap - worst < GAP_MIN:
                self.amp *= 2
                if self.amp > 2048:
                    raise ValueError("ALiBi slope * context is too large for an exact needle")
        self.gap = self.amp * unit_gap
        assert self.gap >= GAP_MIN

        # ---- caches (natural layout first), k, v ----
        K = torch.full((Bc, Hkv, Lmax, Dh), float("nan"), dtype=dt)
        V = torch.full((Bc, Hkv, Lmax, Dh), float("nan"), dtype=dt)
        k = torch.empty(B, Hkv, Dh, dtype=dt)
        v = torch.empty(B, Hkv, Dh, dtype=dt)
        for b in range(B):
            tl = T[b]
            pos = np.arange(first[b], tl + 1)  # the last one is the current token
            x = pos[None, :] + self.salt[b][:, None]
            Kb = code(x, Dh)  # [Hkv, n, Dh]
            Vb = vrow(np.broadcast_to(pos, x.shape), np.broadcast_to(self.salt[b][:, None], x.shape), Dh, fixed_sign)
            for kvh in range(Hkv):
                for p, row in self._overrides(b, kvh).items():
                    Kb[kvh, p - first[b]] = row
            k[b] = torch.from_numpy(Kb[:, -1]).to(dt)
            v[b] = torch.from_numpy(Vb[:, -1]).to(dt)
            if len(pos) > 1:
                Kc = torch.from_numpy(Kb[:, :-1])
                if self.rot:
                    Kc = A.rotate(Kc.double(), tl, self.rot, self.base, self.scale, self.neox, emulate_fp32=False)
                slots = torch.from_numpy(pos[:-1] % Lmax)
                K[b][:, slots] = Kc.to(dt)
                V[b][:, slots] = torch.from_numpy(Vb[:, :-1]).to(dt)
        self.k, self.v = k, v
        self.kc, self.vc = A.to_ft_k_cache(K), V
        self.kw = dict(timestep=t, rotary_embedding_dim=self.rot, rotary_base=self.base, rotary_scale=self.scale,
                       neox_rotary_style=self.neox)

    def _overrides(self, b: int, kvh: int):
        """position -> key row (float32 [Dh]) that replaces the position's own code."""
        Dh, s = self.spec["Dh"], int(self.salt[b, kvh])
        if self.kind == "pair":
            p1, p2 = self.spec["pair"]
            return {p2: code(p1 + s, Dh)}
        if self.kind in ("stair", "mirror"):
            pstar, pd = int(self.needles[0, b, kvh * self.G]), int(self.decoy[b, kvh])
            xs = pstar + s
            out = {}
            for j in range(16):  # every attended one-bit neighbour of the needle moves far away ...
                p = (xs ^ (1 << j)) - s
                if self.first[b] <= p <= self.T[b]:
                    out[p] = -code(xs, Dh)
            out[pd] = code(xs ^ (1 << ((b + kvh) % 16)), Dh)  # ... and the decoy sits exactly one gap below the needle
            return out
        return {}

    def q(self, call: int) -> torch.Tensor:
        Dh = self.spec["Dh"]
        salt_h = np.repeat(self.salt, self.G, axis=1)  # [B, H]
        return torch.from_numpy(self.amp * code(self.needles[call] + salt_h, Dh)).to(self.dtype)

    def target(self, call: int) -> torch.Tensor:
        Dh = self.spec["Dh"]
        salt_h = np.repeat(self.salt, self.G, axis=1)
        tg = vrow(self.needles[call], salt_h, Dh, self.fixed_sign)
        if self.kind == "pair":
            p2 = np.full_like(self.needles[call], self.spec["pair"][1])
            tg = (tg + vrow(p2, salt_h, Dh, True)) / 2
        return torch.from_numpy(tg).to(self.dtype)

    def expected_caches(self, k_written: torch.Tensor):
        """The caches after the call: the slot t % Lmax of rows < B holds k_written [B, Hkv, Dh] / v, all else untouched."""
        kc, vc = self.kc.clone(), self.vc.clone()
        Dh, Lmax = self.spec["Dh"], self.spec["Lmax"]
        for b in range(self.spec["B"]):
            ti = self.T[b] % Lmax
            kc[b, :, :, ti, :] = k_written[b].reshape(-1, Dh // 8, 8)
            vc[b, :, ti, :] = self.v[b]
        return kc, vc


def decode_mut(case: Case, call: int, mutant=None):
    """tests/attn_oracle.decode restated with one fault switched in (mutant None: the same arithmetic, fault-free).
    Returns out float64 [B, H, Dh]."""
    s = case.spec
    B, H, Hkv, Dh, Lmax = s["B"], s["H"], s["Hkv"], s["Dh"], s["Lmax"]
    G = case.G
    q, k, v, kc, vc = case.q(call), case.k, case.v, case.kc, case.vc
    rot, base, scale, neox = case.rot, case.base, case.scale, case.neox
    if mutant == "rot_style":
        neox = not neox
    elif mutant == "rot_dim":
        rot = Dh // 2 if rot == Dh else Dh
    elif mutant == "rot_base":
        base = 500000.0 if base == 10000.0 else 10000.0
    elif mutant == "rot_scale":
        scale = 0.5 if scale == 1.0 else 1.0
    out = torch.zeros(B, H, Dh, dtype=torch.float64)
    drop = int(case.needles[call, 0, 0])
    for b in range(B):
        t = case.T[b]
        first = max(0, t + 1 - Lmax) + {"first-1": -1, "first+1": 1}.get(mutant, 0)
        pos = np.arange(first, t + 1)
        if mutant == "drop" and b == 0:
            pos = pos[pos != drop]
        if len(pos) == 0:
            continue  # (nothing attended: the output row stays zero)
        idx = pos % Lmax
        qr = A.rotate(q[b], t, rot, base, scale, neox)
        kr = A.rotate(k[b], t, rot, base, scale, neox)
        cb = (b + 1) % case.Bc if mutant == "row+1" else b
        for kvh in range(Hkv):
            ck = (kvh + 1) % Hkv if mutant == "kvh+1" else kvh
            K = A.k_cache_rows(kc, cb, ck, idx).double()
            V = vc[cb, ck][idx].double()
            if mutant != "stale" and pos[-1] == t:
                K[-1], V[-1] = kr[kvh].double(), v[b, kvh].double()
            for g in range(G):
                h = kvh * G + g
                sc = (K @ qr[h].double()) / np.sqrt(Dh)
                if case.alibi is not None:
                    sc = sc + float(case.alibi[h]) * torch.from_numpy((pos - t).astype(np.float64))
                p = torch.exp(sc - sc.max())
                out[b, h] = (p @ V) / (p.sum() + 1e-6)
    return out


def mutant_applies(case: Case, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    s = case.spec
    if mutant == "kvh+1":
        return s["Hkv"] > 1
    if mutant == "row+1":
        return case.Bc > 1
    if mutant == "first+1":  # drops the first attended position: seen where a needle (or pair member) sits on it
        return any((case.needles[0, b] == case.first[b]).any() for b in range(s["B"]))
    if mutant.startswith("rot_"):
        # a needle at p* = t cannot see rotation, nor can a context below 63 positions (the angles are too small)
        return case.rot > 0 and any(case.T[b] >= 63 and (case.needles[0, b] != case.T[b]).any() for b in range(s["B"]))
    return True  # drop (of call 0's first needle), stale (the slot holds NaN), first-1 (reads a NaN slot)


# ------------------------------------------------------------------------------------------------------------------------
# the large-cache construction (torch ops on any device): a random +-1 background, code rows only at the needles and their
# one-bit neighbours, needles in the last batch row and KV head
# ------------------------------------------------------------------------------------------------------------------------
LARGE_SALT = 17


def build_large(device, dtype, B: int, Hkv: int, G: int, Dh: int, Lmax: int, seed: int = 1):
    """Returns (q, k, v, kc, vc, t, needles [G], target [G, Dh]): the heads of the last (batch row, KV head) carry the needles."""
    t = Lmax - 1
    H = Hkv * G
    assert t + LARGE_SALT + 1 < 65536
    gen = torch.Generator(device=device).manual_seed(seed)

    def pm1(*shape):
        return (torch.randint(0, 2, shape, device=device, dtype=torch.int8, generator=gen) * 2 - 1).to(dtype)

    kc = torch.empty(B, Hkv, Dh // 8, Lmax, 8, dtype=dtype, device=device)
    vc = torch.empty(B, Hkv, Lmax, Dh, dtype=dtype, device=device)
    for b in range(B):  # one row at a time: the int8 draw stays small
        kc[b] = pm1(Hkv, Dh // 8, Lmax, 8)
        vc[b] = pm1(Hkv, Lmax, Dh)
    q = AMP * pm1(B, H, Dh)
    k, v = pm1(B, Hkv, Dh), pm1(B, Hkv, Dh)
    edges = edge_positions(0, t, 1, Lmax, Lmax)
    needles = np.asarray(_fill(edges, 0, t, G)[:G], dtype=np.int64)
    if G >= 4:
        needles[3] = t  # the current token is always one of them
    b, kvh = B - 1, Hkv - 1
    rows = set()
    for p in needles.tolist():
        rows.add(p)
        for j in range(16):
            n = ((p + LARGE_SALT) ^ (1 << j)) - LARGE_SALT
            if 0 <= n <= t:
                rows.add(n)
    rows = np.asarray(sorted(rows), dtype=np.int64)
    Kr = torch.from_numpy(code(rows + LARGE_SALT, Dh)).to(dtype)
    Vr = torch.from_numpy(vrow(rows, np.full_like(rows, LARGE_SALT), Dh, False)).to(dtype)
    cur = rows == t
    k[b, kvh] = Kr[int(np.nonzero(cur)[0][0])].to(device) if cur.any() else torch.from_numpy(code(t + LARGE_SALT, Dh)).to(dtype).to(device)
    v[b, kvh] = torch.from_numpy(vrow(np.asarray(t), np.asarray(LARGE_SALT), Dh, False)).to(dtype).to(device)
    keep = torch.from_numpy(rows[~cur])
    kc[b, kvh][:, keep.to(device), :] = Kr[~torch.from_numpy(cur)].reshape(-1, Dh // 8, 8).permute(1, 0, 2).to(device)
    vc[b, kvh][keep.to(device)] = Vr[~torch.from_numpy(cur)].to(device)
    q[b, kvh * G:(kvh + 1) * G] = torch.from_numpy(AMP * code(needles + LARGE_SALT, Dh)).to(dtype).to(device)
    target = torch.from_numpy(vrow(needles, np.full_like(needles, LARGE_SALT), Dh, False)).to(dtype)
    return q, k, v, kc, vc, t, needles, target


# ------------------------------------------------------------------------------------------------------------------------
# the parameter sets
# ------------------------------------------------------------------------------------------------------------------------
GROUPS = ((1, 32), (2, 8), (3, 2), (4, 8), (5, 1), (6, 2), (7, 8), (8, 1), (12, 2), (16, 8), (32, 1), (2, 1), (5, 8), (12, 1), (3, 8))
ROT_PARAMS = ((10000.0, 1.0), (500000.0, 0.5))
ROT_LMAX = {63: 128, 1000: 512, 4095: 4096, 32767: 32768}


def _cases():
    out = []

    def add(name, group, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", group=group, dtype=dt))

    # every attended position a needle exactly once
    add("exh-t4095-L4096", "exhaust", B=8, H=32, Hkv=8, Dh=128, Lmax=4096, t=4095, positions="exhaust")
    add("exh-t5000-L1024", "exhaust", B=8, H=32, Hkv=8, Dh=64, Lmax=1024, t=5000, positions="exhaust")
    add("exh-t8191-B1-Hkv2", "exhaust", B=1, H=64, Hkv=2, Dh=64, Lmax=8192, t=8191, positions="exhaust")
    # edge sweep at 32 k: both sides of every split edge, tile edges, the ends, the wrap pair
    add("edge32k-L32768", "edges32k", B=1, H=32, Hkv=1, Dh=128, Lmax=32768, t=32767)
    add("edge32k-L4096", "edges32k", B=1, H=32, Hkv=1, Dh=128, Lmax=4096, t=32767)
    add("edge-t30000-L4096", "edges32k", B=1, H=32, Hkv=1, Dh=128, Lmax=4096, t=30000)  # (t = 32767 ends in slot Lmax - 1: no wrap)
    add("edge32k-L32768-tiles", "edges32k", B=4, H=32, Hkv=4, Dh=64, Lmax=32768, t=32767, positions="all_edges")
    # group sizes x head dims, each query head of a KV head with its own needle; non-power-of-two Lmax, every other one circular
    for i, Dh in enumerate(range(32, 257, 16)):
        G, Hkv = GROUPS[i]
        add(f"grp-G{G}-Hkv{Hkv}-Dh{Dh}", "groups", B=2, Bc=3, H=G * Hkv, Hkv=Hkv, Dh=Dh, Lmax=1000, t=(700, 1700)[i % 2])
    for Dh in (32, 80, 128, 256):  # the head dims of the issue once more over many splits
        add(f"dh{Dh}-t8191", "groups", B=1, H=8, Hkv=2, Dh=Dh, Lmax=8192, t=8191)
    # one block walks all 16 tiles (B * Hkv >= 256: one split)
    add("onesplit-t4095", "onesplit", B=32, H=16, Hkv=8, Dh=64, Lmax=4096, t=4095, positions="all_edges")
    # device lengths under a loose host bound
    add("lens", "lens", B=6, Bc=7, H=8, Hkv=2, Dh=128, Lmax=8192, t=8191, lens=("zero", "small", "edge-1", "edge", "max", "edge2"))
    add("lens-graph-a", "lens", B=6, Bc=6, H=8, Hkv=2, Dh=128, Lmax=8192, t=8191, lens=("zero", "small", "edge-1", "edge", "max", "edge2"))
    add("lens-graph-b", "lens", B=6, Bc=6, H=8, Hkv=2, Dh=128, Lmax=8192, t=8191, lens=("max", "edge", "mid", "zero", "small", "edge-1"), shift=3)
    # running-max paths
    for kind in ("stair", "mirror"):
        add(f"{kind}-onesplit", "stair", B=32, H=16, Hkv=8, Dh=32, Lmax=4096, t=4095, kind=kind)
        add(f"{kind}-4splits", "stair", B=8, H=16, Hkv=8, Dh=64, Lmax=4096, t=4095, kind=kind)
    # pairs (B * Hkv = 64 at 4 k: 4 splits of 4 tiles)
    big = dict(B=8, H=16, Hkv=8, Dh=64, kind="pair")
    add("pair-in-tile", "pair", Lmax=4096, t=4095, pair=(10, 20), **big)
    add("pair-tile-edge", "pair", Lmax=4096, t=4095, pair=(255, 256), **big)
    add("pair-split-edge", "pair", Lmax=4096, t=4095, pair=(1023, 1024), **big)
    add("pair-first-t", "pair", Lmax=4096, t=4095, pair=(0, 4095), **big)
    add("pair-wrap", "pair", Lmax=1024, t=5000, pair=(4095, 4096), **big)
    add("pair-first-t-wrap", "pair", Lmax=1024, t=5000, pair=(3977, 5000), **big)
    add("pair-first-t-wrap-L1000", "pair", Lmax=1000, t=1700, pair=(701, 1700), B=2, H=24, Hkv=2, Dh=128, kind="pair")  # 3 head groups per KV head
    # rotary
    for rot in ROTS[1:]:
        for base, scale in ROT_PARAMS:
            for t in (63, 1000, 4095, 32767):
                for Dh in (64, 128):
                    B, Hkv, G = (1, 1, 8) if t == 32767 else (2, 2, 4)
                    add(f"rot-{rot}-b{base:g}-s{scale:g}-t{t}-Dh{Dh}", "rotary", B=B, Bc=B + 1, H=G * Hkv, Hkv=Hkv, Dh=Dh, Lmax=ROT_LMAX[t],
                        t=t, rot=rot, base=base, scale=scale)
    # ALiBi: one short, one multi-split context
    add("alibi-t200", "alibi", B=2, H=8, Hkv=2, Dh=128, Lmax=256, t=200, alibi=True)
    add("alibi-t4095", "alibi", B=1, H=16, Hkv=2, Dh=64, Lmax=4096, t=4095, alibi=True)
    add("alibi-t1700-rot", "alibi", B=2, H=8, Hkv=2, Dh=128, Lmax=1000, t=1700, alibi=True, rot="full_neox")
    return out


CASES = _cases()
LARGE = dict(B=33, Hkv=16, G=8, Dh=128, Lmax=32768)       # 33 * 16 * 32768 * 128 = 2.2e9 > 2^31 elements per cache
LARGE_SMALL = dict(B=3, Hkv=2, G=8, Dh=128, Lmax=512)     # the same construction at a size the CPU oracle can walk


def case_id(spec) -> str:
    return spec["name"]
