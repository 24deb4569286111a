"""Ragged needle batches for attention over a natural-layout KV cache with per-sequence lengths on the device (awq_attn_kvcache).

Row b of a batch is a B = 1 `tests.attn_prefill_cases.Case` of the batch's (H, Hkv, Dh, Sq, dtype) with a length Sk_b of its own: its
k / v are copied into cache[b, :Sk_b] of a [B, lmax, Hkv, Dh] cache that holds NaN everywhere else, q and the targets are stacked.  An
inactive row (length None) has a q of its own, an all-NaN cache row and a zero target.  seqlens_k and seqlen_offset are chosen so that
seqlens_k[b] + seqlen_offset = Sk_b; an inactive row holds -1 (the batches that have one use seqlen_offset <= 1, so that it stays below
1).  Every mode of Case is one-hot (or an exact mean of two rows), so a target does not depend on how the keys are cut, nor on the
bound the plan was made from: tests/test_attention_kvcache_host.py proves on the CPU that `ragged` below -- per sequence
`tests.attn_splitkv_oracle.splitkv` on cache[b, :Sk_b], zeros for an inactive row -- returns every target bit for bit, and that each of its
mutants does not.  tests/test_gpu_attention_kvcache.py runs the same batches through the kernels with the chunk forced to 64 keys.

`mutant` switches one fault in:
    len+1 / len-1   every sequence is one key longer / shorter than its entry says
    lenswap         sequence b uses the length of sequence b + 1 (cyclic)
    bound           every sequence uses max_seqlen_k in the place of its own length
    shiftmax        the causal shift is taken from the bound (max_seqlen_k - Sq) while the keys end at Sk_b
    inactive-nan    an inactive sequence is not zeroed
"""
from __future__ import annotations

import torch

from tests import attn_splitkv_oracle as S
from tests.attn_prefill_cases import Case

CHUNK = S.CHUNK
MUTANTS = ("len+1", "len-1", "lenswap", "bound", "shiftmax", "inactive-nan")
# (Sq, lengths, bound): None = an inactive row.  Sq 1 meets a tight and a loose bound; (8, 9 | 32, 33): rows whose first keys are masked;
# 65 / 129 / 193 / 257: one key behind a chunk edge; 64: exactly one chunk; 1: a single key
SHAPES = (
    (1, (65, 129, 1, 64, 257, None), 257),
    (1, (65, 129, 1, 64, 257, None), 1024),
    (8, (193, 8, 72, 257, 9), 257),
    (32, (257, 32, 100, 33), 257),
)
PAD = 7  # cache rows behind the bound (NaN like every row that holds no key)


class Batch:
    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        H, Hkv, Dh, Sq = s["H"], s["Hkv"], s["Dh"], s["Sq"]
        self.lens, self.bound, self.offset = tuple(s["lens"]), s["bound"], s["offset"]
        self.mode = mode = s["mode"]
        self.causal = s.get("causal", True)
        self.lmax = self.bound + PAD
        B = len(self.lens)
        assert all(n is None or 1 <= n <= self.bound for n in self.lens) and Sq * (H // Hkv) <= 128
        assert self.offset <= 1 or None not in self.lens
        self.rows = []
        nan = float("nan")
        self.k_cache = torch.full((B, self.lmax, Hkv, Dh), nan, dtype=dt)
        self.v_cache = torch.full((B, self.lmax, Hkv, Dh), nan, dtype=dt)
        self.q = torch.empty(B, Sq, H, Dh, dtype=dt)
        self.target = torch.zeros(B, Sq, H, Dh, dtype=dt)
        self.scale = None
        for b, n in enumerate(self.lens):
            row = dict(B=1, H=H, Hkv=Hkv, Dh=Dh, Sq=Sq, Sk=n if n is not None else Sq + b, dtype=dt, causal=self.causal, padq=0, padk=0)
            if mode == "pair" and n is not None and n >= 65:
                row.update(mode="pair", pair=(63, 64))
            elif mode == "pair" or n is None:  # too short for the pair, or only a q is needed: the diagonal
                row.update(mode="negscale" if mode == "negscale" else "diag")
            elif mode == "decoy":
                row.update(mode="decoy", call=s["call"])
            else:
                row.update(mode=mode)
            case = Case(row)
            self.rows.append(case if n is not None else None)
            self.q[b] = case.q[0]
            self.scale = case.scale
            if n is not None:
                self.k_cache[b, :n] = case.k[0]
                self.v_cache[b, :n] = case.v[0]
                self.target[b] = case.target[0]
        self.seqlens_k = torch.tensor([-1 if n is None else n - self.offset for n in self.lens], dtype=torch.int32)
        self.decoys = sum(c.decoys for c in self.rows if c is not None and c.mode == "decoy")

    def total(self):
        """Sk_b as the kernels form it."""
        return [int(n) + self.offset for n in self.seqlens_k]


def ragged(batch: Batch, chunk: int = CHUNK, mutant=None):
    """The ragged call restated in torch on the CPU: out T [B, Sq, H, Dh]."""
    B, Sq = batch.q.shape[0], batch.q.shape[1]
    tot = batch.total()
    out = torch.zeros_like(batch.q)
    for b in range(B):
        n = tot[(b + 1) % B] if mutant == "lenswap" else tot[b]
        n += {"len+1": 1, "len-1": -1}.get(mutant, 0)
        if mutant == "bound":
            n = batch.bound
        if n < 1 or n > batch.bound:
            if mutant == "inactive-nan":
                out[b] = float("nan")
            continue
        q, k, v = batch.q[b:b + 1], batch.k_cache[b:b + 1, :n], batch.v_cache[b:b + 1, :n]
        if mutant == "shiftmax" and batch.causal:
            for i in range(Sq):  # one row at a time: a single causal row attends every key it is given
                lim = min(i + batch.bound - Sq, n - 1)
                if lim >= 0:
                    out[b, i] = S.splitkv(q[:, i:i + 1], k[:, :lim + 1], v[:, :lim + 1], batch.scale, True, chunk=chunk)[0, 0]
        else:
            out[b] = S.splitkv(q, k, v, batch.scale, batch.causal, chunk=chunk)[0]
    return out


def mutant_applies(batch: Batch, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    live = [n for n in batch.lens if n is not None]
    if mutant == "len+1":         # cache row Sk_b holds NaN and the (shifted) mask lets the last query row attend it
        return True
    if mutant == "len-1":         # the last attended key of every row is lost: seen where it is the target
        return batch.mode in ("diag", "negscale")
    if mutant == "lenswap":       # a longer neighbour brings NaN rows in, a shorter one loses the diagonal; an inactive neighbour zeroes
        return len(set(batch.lens)) > 1 and (batch.mode in ("diag", "negscale") or None in batch.lens or
                                             any(live[(i + 1) % len(live)] > n for i, n in enumerate(live)))
    if mutant == "bound":         # rows Sk_b .. bound - 1 of the cache hold NaN
        return any(n < batch.bound for n in live)
    if mutant == "shiftmax":      # a sequence shorter than the bound attends its first masked key: seen where a decoy sits there
        return batch.causal and any(c is not None and c.mode == "decoy" and c.decoys > 0 and n < batch.bound
                                    for c, n in zip(batch.rows, batch.lens))
    if mutant == "inactive-nan":
        return None in batch.lens
    raise ValueError(mutant)


def _cases():
    out = []

    def add(name, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    n = 0
    for Sq, lens, bound in SHAPES:
        modes = [("diag", None), ("scatter", None), ("edges", None), ("negscale", None), ("pair", None)]
        if Sq > 1:  # (one query row has no masked key to put a decoy on)
            modes += [("decoy", c) for c in range(3)]
        groups = (1, 4, 8) if Sq * 8 <= 128 else (1, 4)
        for mode, call in modes:
            # G, Hkv and Dh take turns; the offset alternates between "lengths before the store" (Sq) and total lengths (0)
            G, Hkv, Dh = groups[n % len(groups)], (2, 1)[(n // 2) % 2], (64, 128)[(n // 3) % 2]
            offset = (Sq, 0)[n % 2] if None not in lens else (1, 0)[n % 2]
            tag = mode if call is None else f"{mode}{call}"
            add(f"{tag}-Sq{Sq}-bound{bound}-G{G}", H=G * Hkv, Hkv=Hkv, Dh=Dh, Sq=Sq, lens=lens, bound=bound, offset=offset, mode=mode, call=call)
            n += 1
    return out


CASES = _cases()


def case_id(spec) -> str:
    return spec["name"]
