"""Needle cases for the encoder-tower attention kernel (csrc/awq_attn_tower_cdna4.hip): head dim 72 in the dense form, and sequences
packed behind cu_seqlens at head dims 64 and 72.  Every case has an answer known to the bit; tests/test_attention_tower_host.py proves
on the CPU that the float64 oracle alone returns it (and that oracle-level faults do not), tests/test_gpu_attention_tower.py runs the
same entries through the kernel.

Dense cases are tests/attn_prefill_cases.Case at Dh = 72, causal = False (its modes and its NaN padding carry over).  code() spells a
position's 16 bits over the columns d % 16, so at Dh = 72 the bits 0 .. 7 own five columns and the bits 8 .. 15 four: one flipped bit
costs at least 2 * 32 * (72 // 16) / sqrt(72) = 30.2 >= GAP_MIN.

TailCase (Dh = 72 only): q and k are zero except the columns 64 .. 71, where key j carries +-1 by the 8 bits of j and the query 32 x the
code of its target; softmax_scale = 1.  The sought key scores 8 * 32 = 256, any other at most 6 * 32 = 192.  A kernel that drops or
garbles the ninth 16-byte chunk scores every key alike and answers with the mean of V.

poisoned(): a dense fused case with three heads whose heads 0 and 2 are NaN in q, k and v: head 1 must still be exact, which it is
not if the padding of the reduction dimension (columns 72 .. 79) is taken from the next head.

VarlenCase: a packed qkv [rows, 3, H, Dh] and cu_seqlens.  Key j of sequence s, head h is code(j + salt(s, h)): the salt depends on the
sequence, so no two sequences share a key.  The non-empty sequences are numbered n = 0, 1, ..; an EVEN one aims rows at its own first
and last key while the row next door -- the last key of its left neighbour, the first key of its right neighbour -- carries that same
code as a decoy (its V row is its own): one key too many on either side halves the weight.  An ODD one (whose two end keys are those
decoys) aims inside [1, len - 2].  Besides the ends, rows walk a hash of the range and both sides of every 64-key edge.  Rows of the
allocation beyond cu_seqlens[-1] hold NaN, and max_seqlen may exceed the longest sequence.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import attn_prefill_cases as P
from tests import attn_prefill_oracle as O
from tests.attn_cases import AMP, GAP_MIN, code, salt_of, vrow

KV_TILE = 64
MUTANTS = ("end+1", "start-1", "seq+1", "maxlen", "kvh+1", "droptile", "unscaled", "tail")
DTYPES = (torch.float16, torch.bfloat16)


def gap(Dh: int) -> float:
    """The least score gap between the sought key and a key whose position differs in one bit."""
    return 2.0 * AMP * (Dh // 16) / math.sqrt(Dh)


assert gap(72) >= GAP_MIN and gap(64) >= GAP_MIN


# ------------------------------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------------------------------
def _dense():
    out = []

    def add(name, **kw):
        for dt in DTYPES:
            out.append(dict(dict(Dh=72, causal=False, fused=True), **kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    for S in (1, 63, 64, 65, 127, 129, 200):
        add(f"edges-S{S}", B=1, H=3, Hkv=3, Sq=S, Sk=S, mode="edges")
        add(f"scatter-S{S}", B=2, H=4, Hkv=2, Sq=S, Sk=S, mode="scatter")
    add("scatter-S729-tower", B=1, H=16, Hkv=16, Sq=729, Sk=729, mode="scatter")  # SigLIP-so400m's own shape
    add("edges-S729", B=1, H=2, Hkv=1, Sq=729, Sk=729, mode="edges")
    for S in (200, 729):
        for mode in ("zero", "diag", "negscale"):
            add(f"{mode}-S{S}", B=1, H=4, Hkv=2, Sq=S, Sk=S, mode=mode)
    add("scatter-100x333", B=2, H=4, Hkv=2, Sq=100, Sk=333, mode="scatter")
    add("edges-333x100", B=2, H=4, Hkv=2, Sq=333, Sk=100, mode="edges", fused=False)
    add("scatter-B3", B=3, H=2, Hkv=1, Sq=65, Sk=65, mode="scatter")
    add("pair-tile-edge", B=1, H=4, Hkv=2, Sq=200, Sk=200, mode="pair", pair=(63, 64))
    add("pair-far-S65", B=1, H=2, Hkv=2, Sq=65, Sk=65, mode="pair", pair=(0, 64))
    add("pair-far-S729", B=1, H=2, Hkv=1, Sq=729, Sk=729, mode="pair", pair=(0, 728))
    return out


DENSE = _dense()


def dense_case(spec) -> P.Case:
    assert spec["Dh"] == 72 and not spec["causal"]
    return P.Case(spec)


def poisoned(dtype) -> P.Case:
    """A fused dense case of three heads; heads 0 and 2 of q, k and v become NaN.  Only head 1 of the target is meaningful."""
    case = P.Case(dict(name="poisoned", dtype=dtype, Dh=72, causal=False, fused=True, B=2, H=3, Hkv=3, Sq=200, Sk=200, mode="scatter"))
    for t in (case.q, case.k, case.v):
        t[:, :, 0] = float("nan")
        t[:, :, 2] = float("nan")
    return case


class TailCase:
    """See the head of the file.  q [B, Sq, H, 72], k / v [B, Sk, H, 72] contiguous; scale 1."""
    Dh = 72

    def __init__(self, dtype, B=1, H=2, Sq=100, Sk=256):
        assert Sk <= 256
        self.dtype, self.scale, self.causal = dtype, 1.0, False
        i, h, b = np.arange(Sq)[None, :, None], np.arange(H)[None, None, :], np.arange(B)[:, None, None]
        self.tgt = tgt = ((i * 2654435761 + h * 40503 + b * 7 + 977) % (2 ** 31)) % Sk          # [B, Sq, H]
        bits = lambda x: (1 - 2 * ((np.asarray(x)[..., None] >> np.arange(8)) & 1)).astype(np.float32)
        Q = np.zeros((B, Sq, H, 72), np.float32)
        K = np.zeros((B, Sk, H, 72), np.float32)
        Q[..., 64:] = AMP * bits(tgt)
        K[..., 64:] = bits(np.broadcast_to(np.arange(Sk)[None, :, None], (B, Sk, H)))
        salt = np.broadcast_to(13 + 7919 * (b * H + h), (B, Sk, H))
        V = vrow(np.broadcast_to(np.arange(Sk)[None, :, None], (B, Sk, H)), salt, 72, False)
        T = vrow(tgt, np.broadcast_to(13 + 7919 * (b * H + h), tgt.shape), 72, False)
        self.q, self.k, self.v = (torch.from_numpy(x).to(dtype) for x in (Q, K, V))
        self.target = torch.from_numpy(T).to(dtype)
        assert torch.equal(self.target.double(), torch.from_numpy(T.astype(np.float64)))

    def to(self, device):
        return self.q.to(device), self.k.to(device), self.v.to(device)


# ------------------------------------------------------------------------------------------------------------------------
# varlen
# ------------------------------------------------------------------------------------------------------------------------
class VarlenCase:
    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        self.lens = lens = list(s["lens"])
        self.H, self.Dh = H, Dh = s["H"], s["Dh"]
        self.max_seqlen = s.get("max_seqlen", max(lens))
        assert self.max_seqlen >= max(lens) and gap(Dh) >= GAP_MIN
        self.pad = pad = s.get("pad", 3)
        self.cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.total = total = int(self.cu[-1])
        self.rows = total + pad
        self.nonempty = ne = [i for i, n in enumerate(lens) if n > 0]
        nseq = len(lens)
        self.salt = np.array([[salt_of(i, h, H, max(lens)) for h in range(H)] for i in range(nseq)], dtype=np.int64)
        for h in range(H):  # no two sequences share a code
            spans = sorted((int(self.salt[i, h]), int(self.salt[i, h]) + lens[i]) for i in ne)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] < 65536

        K = np.zeros((total, H, Dh), np.float32)
        V = np.zeros((total, H, Dh), np.float32)
        Q = np.zeros((total, H, Dh), np.float32)
        T = np.zeros((total, H, Dh), np.float32)
        self.tgt = np.zeros((total, H), np.int64)  # in-sequence position of the sought key
        hh = np.arange(H, dtype=np.int64)
        self.decoys = {"left": 0, "right": 0}
        for n, i in enumerate(ne):
            L, b0 = lens[i], int(self.cu[i])
            j = np.arange(L, dtype=np.int64)
            salt = self.salt[i]                                                      # [H]
            K[b0:b0 + L] = code(j[:, None] + salt[None, :], Dh)
            V[b0:b0 + L] = vrow(np.broadcast_to(j[:, None], (L, H)), np.broadcast_to(salt[None, :], (L, H)), Dh, False)
            if n % 2 == 0:
                lo, hi = 0, L - 1
            else:
                assert L >= 3, "an odd-numbered sequence lends both its end keys to its neighbours"
                lo, hi = 1, L - 2
            m = j[:, None] + hh[None, :]                                             # [L, H]
            span = hi - lo + 1
            scatter = lo + ((j[:, None] * 2654435761 + hh[None, :] * 40503 + 977 + 31 * i) % (2 ** 31)) % span
            edge = np.clip(KV_TILE * ((m // 8) % (hi // KV_TILE + 1)) - ((m // 4) & 1), lo, hi)
            tgt = np.select([m % 4 == 0, m % 4 == 1, m % 4 == 2], [scatter, edge, np.full_like(m, lo)], np.full_like(m, hi))
            self.tgt[b0:b0 + L] = tgt
            Q[b0:b0 + L] = AMP * code(tgt + salt[None, :], Dh)
            T[b0:b0 + L] = vrow(tgt, np.broadcast_to(salt[None, :], (L, H)), Dh, False)
        for n, i in enumerate(ne):  # the decoys, after every sequence's own keys
            if n % 2:
                continue
            L, b0 = lens[i], int(self.cu[i])
            if n > 0:
                K[b0 - 1] = code(0 + self.salt[i], Dh)
                self.decoys["left"] += 1
            if n + 1 < len(ne):
                K[b0 + L] = code(L - 1 + self.salt[i], Dh)
                self.decoys["right"] += 1
        qkv = torch.full((self.rows, 3, H, Dh), float("nan"), dtype=dt)
        qkv[:total, 0] = torch.from_numpy(Q)
        qkv[:total, 1] = torch.from_numpy(K)
        qkv[:total, 2] = torch.from_numpy(V)
        self.qkv = qkv
        self.cu_seqlens = torch.from_numpy(self.cu).to(torch.int32)
        self.target = torch.from_numpy(T).to(dt)
        assert torch.equal(self.target.double(), torch.from_numpy(T.astype(np.float64)))


def varlen_oracle(qkv, cu, max_seqlen: int, scale=None, mutant=None, stats: bool = False):
    """float64 statement of flash_attn_varlen_qkvpacked_func(causal=False): qkv [rows, 3, H, Dh] (rows may exceed cu[-1]), cu a list of
    nseq + 1 ints.  Runs tests.attn_prefill_oracle.attention per sequence on the device of qkv.  Returns out [cu[-1], H, Dh] (with
    stats: also A and qk of that oracle, and the key count per row, for its bound).  `mutant` switches one fault in:
        end+1 / start-1   one key too many at either end        seq+1   the next sequence's keys
        maxlen            max_seqlen taken as the length         kvh+1 / droptile (as the dense oracle's)
        tail              the columns >= 64 ignored in q k^T"""
    rows, _, H, Dh = qkv.shape
    cu = [int(x) for x in cu]
    nseq, total = len(cu) - 1, cu[-1]
    out = torch.zeros(total, H, Dh, dtype=torch.float64, device=qkv.device)
    A = torch.zeros_like(out) if stats else None
    qk = torch.zeros(total, H, dtype=torch.float64, device=qkv.device) if stats else None
    q = qkv[:, 0]
    if mutant == "tail":
        q = q.clone()
        q[..., 64:] = 0
    for s in range(nseq):
        b, e = cu[s], cu[s + 1]
        if e <= b:
            continue
        kb, ke = b, e
        if mutant == "end+1":
            ke = min(e + 1, rows)
        elif mutant == "start-1":
            kb = max(b - 1, 0)
        elif mutant == "seq+1":
            kb, ke = cu[(s + 1) % nseq], cu[(s + 1) % nseq + 1]
        elif mutant == "maxlen":
            ke = min(b + max_seqlen, rows)
        if ke <= kb:
            out[b:e] = float("nan")  # nothing attended
            continue
        qe = min(e, b + max_seqlen)  # rows beyond max_seqlen are not computed
        inner = mutant if mutant in ("kvh+1", "droptile") else None
        sc = float(Dh) ** -0.5 if scale is None else scale
        r = O.attention(q[None, b:qe], qkv[None, kb:ke, 1], qkv[None, kb:ke, 2], sc, False, mutant=inner, stats=stats)
        if stats:
            out[b:qe], A[b:qe], qk[b:qe] = r[0][0], r[1][0], r[2][0]
        else:
            out[b:qe] = r[0]
    return (out, A, qk) if stats else out


def _varlen():
    out = []

    def add(name, **kw):
        for dt in DTYPES:
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    for Dh in (64, 72):
        add(f"ragged-Dh{Dh}", lens=[1, 65, 0, 200, 729], H=3, Dh=Dh)
        add(f"ragged-long-max-Dh{Dh}", lens=[1, 65, 0, 200, 729], H=2, Dh=Dh, max_seqlen=800, pad=1)
        add(f"tiles-Dh{Dh}", lens=[64, 64, 64], H=4, Dh=Dh)
        add(f"tiles-long-max-Dh{Dh}", lens=[64, 64, 64], H=2, Dh=Dh, max_seqlen=100)
        add(f"single-Dh{Dh}", lens=[129], H=4, Dh=Dh, max_seqlen=200)
        add(f"empty-ends-Dh{Dh}", lens=[0, 70, 0, 0, 5, 130, 0], H=2, Dh=Dh, max_seqlen=130)
    add("internvit-Dh64", lens=[1025, 1025], H=2, Dh=64)
    return out


VARLEN = _varlen()


def case_id(spec) -> str:
    return spec["name"]


# ------------------------------------------------------------------------------------------------------------------------
# which construction is bound to see which fault (reasons, not measurements)
# ------------------------------------------------------------------------------------------------------------------------
def mutant_applies(case, mutant: str) -> bool:
    if isinstance(case, TailCase):
        return mutant == "tail"  # all of q k^T lives in the columns 64 .. 71; without them every key scores alike
    if isinstance(case, P.Case):
        s = case.spec
        if mutant == "kvh+1":     # another KV head carries another salt
            return s["Hkv"] > 1
        if mutant == "droptile":  # without a mask the last key is the target of every row in these modes
            return case.mode in ("diag", "negscale")
        if mutant == "unscaled":
            return case.mode == "negscale"
        return False              # the sequence faults need cu_seqlens; a one-bit needle survives the loss of the tail columns (gap 30.2)
    n_ne = len(case.nonempty)
    last = case.nonempty[-1]
    if mutant == "end+1":    # the right decoy of sequence n = 0, or the NaN row behind the last sequence
        return n_ne >= 2 or case.pad > 0
    if mutant == "start-1":  # the left decoy of sequence n = 2
        return n_ne >= 3
    if mutant == "seq+1":    # foreign keys (or none at all) unless the next sequence is the same one
        return len(case.lens) >= 2
    if mutant == "maxlen":   # an even-numbered sequence shorter than max_seqlen takes in its right decoy; the last one the NaN rows
        even_short = any(case.lens[i] < case.max_seqlen for n, i in enumerate(case.nonempty) if n % 2 == 0 and n + 1 < n_ne)
        return even_short or (case.lens[last] < case.max_seqlen and case.pad > 0 and sum(case.lens[last + 1:]) == 0)
    if mutant == "kvh+1":
        return case.H > 1
    if mutant == "droptile":  # a sequence of at most one tile loses every key; else a row that aims at the last tile loses its target
        for i in case.nonempty:
            L, b0 = case.lens[i], int(case.cu[i])
            if L <= KV_TILE or (case.tgt[b0:b0 + L] >= (L - 1) // KV_TILE * KV_TILE).any():
                return True
        return False
    if mutant in ("unscaled", "tail"):  # the default scale is used; see above for the tail
        return False
    raise ValueError(mutant)
