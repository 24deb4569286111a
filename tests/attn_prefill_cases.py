"""Needle, decoy and pair cases for prefill attention: inputs whose exact answer is known to the bit (the prefill counterpart of
tests/attn_cases.py, whose code / vrow / salt_of it reuses).

    key of position j        code(keyid[j] + salt); keyid[j] = j unless the mode overrides it; salt depends on (batch row, KV head)
    query of row i, head h   amp * code(tgt(i, h) + salt), amp = 32: the sought key scores 4 sqrt(Dh) >= GAP_MIN above any other
    value row                vrow(j, salt): exact in fp16 / bf16, the signs spell j (a fixed pattern for pair cases)
    target                   vrow(tgt) -- or the exact mean of two rows where two attended positions share the sought key
    padding                  q rows >= Sq and k / v rows >= Sk of the backing allocation hold NaN; with `fused` q, k and v are strided
                             views of one [B, S, (H + 2 Hkv) * Dh] qkv tensor (tinychat's fused_attn.py:242-246)

Modes (tgt and the key overrides):
    diag      tgt = the last attended key of the row (i + Sk - Sq)            sees a mask one too strict, a dropped last tile
    zero      tgt = 0
    scatter   tgt = a hash of (i, h) over the attended keys
    edges     tgt walks both sides of every 64-key tile edge below the row's limit
    decoy     rows i = c (mod 3): the sought key is ALSO placed on the first masked position i + Sk - Sq + 1, where one more attended
              key would halve the weight (c = the case's `call`: three calls cover every row)      sees a mask one too loose
    pair      positions p1 < p2 share a key: rows that attend both return the exact mean
    negscale  q = -amp * code and softmax_scale = -Dh ** -0.5: the same answer only if the scale argument is honoured

CASES is the one list: tests/test_attention_prefill_host.py proves on the CPU that the float64 oracle alone returns the targets
(and that oracle-level faults do not), tests/test_gpu_attention_prefill.py runs the same entries through the kernel, bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.attn_cases import AMP, GAP_MIN, code, salt_of, vrow

KV_TILE = 64


def _limit(i, Sq: int, Sk: int, causal: bool):
    return np.minimum(i + (Sk - Sq), Sk - 1) if causal else np.full_like(i, Sk - 1)


class Case:
    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = s["dtype"]
        B, H, Hkv, Dh, Sq, Sk = s["B"], s["H"], s["Hkv"], s["Dh"], s["Sq"], s["Sk"]
        self.causal = causal = s.get("causal", True)
        self.mode = mode = s.get("mode", "diag")
        self.G = G = H // Hkv
        assert 4.0 * np.sqrt(Dh) >= GAP_MIN and Sk + 8000 * B * Hkv < 10 ** 9
        shift = Sk - Sq
        self.salt = np.array([[salt_of(b, kvh, Hkv, Sk) for kvh in range(Hkv)] for b in range(B)], dtype=np.int64)
        i = np.arange(Sq, dtype=np.int64)
        lim = _limit(i, Sq, Sk, causal)  # [Sq]
        hh = np.arange(H, dtype=np.int64)
        keyid = np.arange(Sk, dtype=np.int64)
        self.fixed_sign = mode == "pair"
        self.pair = None
        if mode in ("diag", "negscale"):
            tgt = np.broadcast_to(lim[:, None], (Sq, H)).copy()
        elif mode == "zero":
            tgt = np.zeros((Sq, H), dtype=np.int64)
        elif mode == "scatter":
            tgt = ((i[:, None] * 2654435761 + hh[None, :] * 40503 + 977) % (2 ** 31)) % (lim[:, None] + 1)
        elif mode == "edges":
            n = i[:, None] + hh[None, :]
            e = KV_TILE * ((n // 2) % (lim[:, None] // KV_TILE + 1)) - (n & 1)
            tgt = np.clip(e, 0, lim[:, None])
        elif mode == "decoy":
            assert causal
            c = s.get("call", 0)
            dec = (i % 3 == c) & (i + shift >= 2) & (i + shift + 1 < Sk)
            t1 = lim.copy()
            after = np.zeros(Sq, dtype=bool)
            after[1:] = dec[:-1]
            t1[after] -= 2  # its own diagonal position holds the previous row's decoy: aim two below (a position with its own code)
            keyid[(i + shift + 1)[dec]] = t1[dec]
            tgt = np.broadcast_to(t1[:, None], (Sq, H)).copy()
            self.decoys = int(dec.sum())
        elif mode == "pair":
            p1, p2 = s["pair"]
            assert 0 <= p1 < p2 < Sk
            keyid[p2] = p1
            tgt = np.where(lim[:, None] >= p1, p1, lim[:, None]) + 0 * hh[None, :]
            self.pair = (p1, p2)
        else:
            raise ValueError(mode)
        assert (tgt >= 0).all() and (tgt <= lim[:, None]).all()
        self.tgt, self.keyid, self.lim = tgt, keyid, lim

        # ---- tensors ----
        amp = -AMP if mode == "negscale" else AMP
        self.scale = -(float(Dh) ** -0.5) if mode == "negscale" else None
        padq, padk = s.get("padq", 3), s.get("padk", 5)
        K = np.stack([np.stack([code(keyid + self.salt[b, kvh], Dh) for kvh in range(Hkv)], 1) for b in range(B)])       # [B, Sk, Hkv, Dh]
        V = np.stack([np.stack([vrow(np.arange(Sk), np.full(Sk, self.salt[b, kvh]), Dh, self.fixed_sign) for kvh in range(Hkv)], 1)
                      for b in range(B)])
        salt_h = np.repeat(self.salt, G, axis=1)  # [B, H]
        Q = amp * code(tgt[None] + salt_h[:, None, :], Dh)                                                                 # [B, Sq, H, Dh]
        T = vrow(np.broadcast_to(tgt[None], (B, Sq, H)), np.broadcast_to(salt_h[:, None, :], (B, Sq, H)), Dh, self.fixed_sign)
        if self.pair is not None:
            p1, p2 = self.pair
            both = (lim >= p2)[None, :, None] & (tgt[None] == p1)
            T2 = vrow(np.full((B, Sq, H), p2), np.broadcast_to(salt_h[:, None, :], (B, Sq, H)), Dh, True)
            T = np.where(both[..., None], (T + T2) / 2, T)
        dt = self.dtype
        self.target = torch.from_numpy(T.astype(np.float32)).to(dt)
        assert torch.equal(self.target.double(), torch.from_numpy(T.astype(np.float64)))  # the targets are exact in T
        if s.get("fused"):
            S = max(Sq + padq, Sk + padk)
            qkv = torch.full((B, S, (H + 2 * Hkv) * Dh), float("nan"), dtype=dt)
            q = qkv[:, :Sq, :H * Dh].view(B, Sq, H, Dh)
            k = qkv[:, :Sk, H * Dh:(H + Hkv) * Dh].view(B, Sk, Hkv, Dh)
            v = qkv[:, :Sk, (H + Hkv) * Dh:].view(B, Sk, Hkv, Dh)
            self.backing = (qkv,)
        else:
            qb = torch.full((B, Sq + padq, H, Dh), float("nan"), dtype=dt)
            kb = torch.full((B, Sk + padk, Hkv, Dh), float("nan"), dtype=dt)
            vb = torch.full((B, Sk + padk, Hkv, Dh), float("nan"), dtype=dt)
            q, k, v = qb[:, :Sq], kb[:, :Sk], vb[:, :Sk]
            self.backing = (qb, kb, vb)
        q.copy_(torch.from_numpy(Q))
        k.copy_(torch.from_numpy(K))
        v.copy_(torch.from_numpy(V))
        self.q, self.k, self.v = q, k, v

    def to(self, device):
        """(q, k, v) on `device` as views of device copies of the NaN-padded backing allocations (same strides)."""
        moved = [t.to(device) for t in self.backing]
        out = []
        for t in (self.q, self.k, self.v):
            for src, dst in zip(self.backing, moved):
                if t.untyped_storage().data_ptr() == src.untyped_storage().data_ptr():
                    out.append(torch.as_strided(dst, t.shape, t.stride(), t.storage_offset()))
                    break
        assert len(out) == 3
        return out


def mutant_applies(case: Case, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    s = case.spec
    if mutant == "mask+1":   # one more key attended: seen where that key is a decoy
        return case.mode == "decoy" and case.decoys > 0
    if mutant == "mask-1":   # the diagonal key not attended: seen where it is the target
        return case.causal and case.mode in ("diag", "negscale")
    if mutant == "topleft":  # rows lose keys i + 1 .. i + Sk - Sq: seen where the target lies there
        return case.causal and s["Sk"] > s["Sq"] and case.mode in ("diag", "negscale")
    if mutant == "kvh+1":
        return s["Hkv"] > 1
    if mutant == "droptile":  # the last tile holds the diagonal of the last rows
        return case.mode in ("diag", "negscale")
    if mutant == "unscaled":
        return case.mode == "negscale"
    raise ValueError(mutant)


def _cases():
    out = []

    def add(name, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    # the issue's soundness shapes, both head dims, every mode
    for Dh in (64, 128):
        for Sq, Sk in ((300, 300), (130, 700)):
            for mode in ("diag", "zero", "scatter", "edges", "negscale"):
                add(f"{mode}-{Sq}x{Sk}-Dh{Dh}", B=1, H=4, Hkv=2, Dh=Dh, Sq=Sq, Sk=Sk, mode=mode)
            for c in range(3):
                add(f"decoy{c}-{Sq}x{Sk}-Dh{Dh}", B=1, H=2, Hkv=1, Dh=Dh, Sq=Sq, Sk=Sk, mode="decoy", call=c)
    # pairs: inside a tile, across a KV tile edge, across the block's q-tile edge, first and last key
    for name, pair in (("in-tile", (10, 20)), ("tile-edge", (63, 64)), ("far", (0, 299)), ("qtile-edge", (127, 128))):
        add(f"pair-{name}", B=1, H=4, Hkv=1, Dh=128, Sq=300, Sk=300, mode="pair", pair=pair)
    add("pair-chunk", B=2, H=2, Hkv=2, Dh=64, Sq=130, Sk=700, mode="pair", pair=(569, 640))
    # square lengths around the tile sizes
    for S in (1, 2, 63, 64, 65, 127, 129, 1000):
        add(f"diag-S{S}", B=1, H=8, Hkv=2, Dh=128, Sq=S, Sk=S, mode="diag")
        add(f"edges-S{S}", B=1, H=4, Hkv=4, Dh=64, Sq=S, Sk=S, mode="edges")
    add("diag-S4096", B=1, H=2, Hkv=1, Dh=128, Sq=4096, Sk=4096, mode="diag")
    add("edges-S4096", B=1, H=2, Hkv=2, Dh=64, Sq=4096, Sk=4096, mode="edges")
    # chunk prefill shapes
    for Sq, Sk in ((1, 500), (130, 700), (512, 2560)):
        add(f"chunk-scatter-{Sq}x{Sk}", B=1, H=4, Hkv=1, Dh=128, Sq=Sq, Sk=Sk, mode="scatter")
        add(f"chunk-diag-{Sq}x{Sk}", B=1, H=2, Hkv=2, Dh=64, Sq=Sq, Sk=Sk, mode="diag")
    # group sizes and batches, q / k / v as views of one qkv tensor
    for G, Hkv in ((1, 3), (4, 2), (7, 1), (8, 2)):
        for B in (1, 3):
            add(f"grp-G{G}-Hkv{Hkv}-B{B}", B=B, H=G * Hkv, Hkv=Hkv, Dh=(64, 128)[G % 2], Sq=200, Sk=200, mode="scatter", fused=True)
    add("fused-chunk", B=2, H=8, Hkv=2, Dh=128, Sq=130, Sk=700, mode="diag", fused=True)
    add("fused-decoy", B=3, H=4, Hkv=2, Dh=128, Sq=257, Sk=257, mode="decoy", call=1, fused=True)
    # every q tile of the plan: 256 rows (Dh = 128 with B * H * ceil(Sq / 256) >= 512), 128 rows, 64 rows (the short Dh = 64 cases above)
    add("wide128", B=4, H=32, Hkv=8, Dh=128, Sq=520, Sk=520, mode="edges")
    add("wide128-Dh64", B=8, H=32, Hkv=8, Dh=64, Sq=1030, Sk=1030, mode="diag")
    add("wide256", B=8, H=32, Hkv=8, Dh=128, Sq=1030, Sk=1030, mode="diag")
    add("wide256-decoy", B=8, H=32, Hkv=4, Dh=128, Sq=1030, Sk=1100, mode="decoy", call=2)
    # non-causal
    add("full-scatter", B=2, H=4, Hkv=2, Dh=128, Sq=100, Sk=333, mode="scatter", causal=False)
    add("full-longq", B=1, H=4, Hkv=4, Dh=64, Sq=333, Sk=100, mode="edges", causal=False)
    add("full-pair", B=1, H=2, Hkv=1, Dh=128, Sq=70, Sk=130, mode="pair", pair=(5, 129), causal=False)
    return out


CASES = _cases()


def case_id(spec) -> str:
    return spec["name"]
