"""One windowed mixed packed step (awq_attn_varq_window[_kv8], awq_attn_paged_varq_window[_kv8]; csrc/awq_window.hpp), built on
tests/attn_varq_split_cases.py's `Step` / `Pool`: H 8 / Hkv 2 (G = 4), max_seqlen_k 512, the split chunk forced to 64, split_min_keys 128,
split_seqlen_q 8, max_seqlen_q 130, pages of 64 / 128 keys, under every window in LEFTS.

STEP lists (new tokens, history before the step); row s of a sequence stands at p = s + history and its window starts at max(0, p - left):

    0  (1, 256)    a decode at p = 256: the start falls at tile offset 0 (left 0, 64), 63 (left 1), 1 (left 63, 191), in the second page of
                   either size (left 191: key 65 at 64-key pages; left 100: key 156 at 128-key pages) and before key 0 (left 511).
                   Sk_b = 257 >= 128 > keys_b for every left <= 126: the sequence `rule-sk` routes differently
    1  (8, 292)    a burst of 8 rows over 300 keys
    2  (70, 64)    a 70-row chunk that crosses a 64-row q tile
    3  (130, 170)  a 130-row chunk over 300 keys: at left 100 the rows of one q tile start in tiles 1 .. 3 and whole tiles are skipped per wave
    4  (0, 500)    Sq_b = 0
    5  (1, -1)     an inactive slot
    6  (2, 511)    beyond the bound: inactive
    7  (3, 509)    fills the bound exactly
    8  (1, 127)    Sk_b = 128, the floor itself: taken as soon as the window reaches key 0
    9  (4, 2)      a short sequence: every start before key 0

TAKEN[left] is the route of every sequence under split_min_keys 128, written down by hand from keys_b = min(Sk_b, left + Sq_b):
    left <= 100: keys_b of sequences 0, 1, 7, 8 is at most 108 -- nobody is taken;  left 191: 192, 199, 194, 128;  left 511: 257, 300, 512, 128.
FORCED is the route under split_min_keys 1: every active sequence with at most 8 rows.

Needles keep a boundary fault out of the noise: for the rows NEEDLE_ROWS of a sequence and every left, key p - left (just inside the window)
and key p - left - 1 (just outside) are aligned with the row's query of the KV head's first query head -- a score far above the rest --
and carry a constant V of their own.  A key two rows claim stays with the first."""
from __future__ import annotations

import torch

from tests import attn_varq_split_cases as S
from tests import attn_window_oracle as O

H, HKV, G, BOUND, LMAX, CHUNK = S.H, S.HKV, S.G, S.BOUND, S.LMAX, S.CHUNK
SPLIT_MIN_KEYS, SPLIT_SEQLEN_Q = S.SPLIT_MIN_KEYS, S.SPLIT_SEQLEN_Q
MAX_Q = 130
PAD_ROWS, SENTINEL, PAGE_SIZES = S.PAD_ROWS, S.SENTINEL, S.PAGE_SIZES
LEFTS = (0, 1, 63, 64, 100, 191, 511)
STEP = ((1, 256), (8, 292), (70, 64), (130, 170), (0, 500), (1, -1), (2, 511), (3, 509), (1, 127), (4, 2))
_NONE = (False,) * 10
_LONG = (True, True, False, False, False, False, False, True, True, False)
TAKEN = {0: _NONE, 1: _NONE, 63: _NONE, 64: _NONE, 100: _NONE, 191: _LONG, 511: _LONG}       # by hand, not computed
FORCED = (True, True, False, False, False, False, False, True, True, True)                    # split_min_keys = 1
RULE_SK = (True, True, False, False, False, False, False, True, True, False)                  # what `rule-sk` gives for EVERY left
NEEDLE_ROWS = {0: (0,), 1: (0, 7), 2: (0, 63, 64, 69), 3: (0, 31, 32, 63, 64, 127, 128, 129), 7: (0, 2), 8: (0,), 9: (3,)}
COMBOS = S.COMBOS


def active(b):
    n, h = STEP[b]
    return 0 <= n <= MAX_Q and 1 <= h + n <= BOUND


def routes(left, floor=SPLIT_MIN_KEYS, mutant=None, before=True):
    return tuple(O.takes(n, h if before else h + n, before, left, MAX_Q, BOUND, SPLIT_SEQLEN_Q, floor, mutant=mutant) for n, h in STEP)


def anchor(b, left):
    """The first key of sequence b's first tile: nothing below it is read."""
    n, h = STEP[b]
    return max(0, h - left) // 64 * 64


class Step(S.Step):
    """S.Step for STEP with this file's max_seqlen_q (the 130-row chunk holds its keys too) and the needles."""

    def __init__(self, dtype, Dh):
        super().__init__(dtype, Dh, STEP)
        g = torch.Generator().manual_seed(4441 + Dh + (1 if dtype == torch.bfloat16 else 0))
        for b, (n, h) in enumerate(STEP):
            if active(b) and self.held[b] != h + n:   # S.active knows S.MAX_Q only
                self.held[b] = h + n
                self.k_cache[b, :h + n] = torch.randn(h + n, HKV, Dh, generator=g).to(dtype)
                self.v_cache[b, :h + n] = (1 + 0.5 * torch.randn(h + n, HKV, Dh, generator=g)).to(dtype)
        self.needles = 0
        for b, rows in NEEDLE_ROWS.items():
            n, h = STEP[b]
            claimed = set()
            for s in rows:
                p = s + h
                for left in LEFTS:
                    for key in (p - left, p - left - 1):
                        if key < 0 or key in claimed:
                            continue
                        claimed.add(key)
                        self.needles += 1
                        for kvh in range(HKV):
                            qv = self.q[self.cu[b] + s, kvh * G].float()
                            self.k_cache[b, key, kvh] = (8.0 * qv / qv.norm()).to(dtype)
                            self.v_cache[b, key, kvh] = (-1.0) ** self.needles * (3.0 + 0.25 * (self.needles % 13))

    def seq(self, b, k=None, v=None):
        """(q, k, v) of sequence b alone, [1, S, heads, Dh]; k / v default to the caches."""
        k = self.k_cache if k is None else k
        v = self.v_cache if v is None else v
        n, h = STEP[b]
        return self.q[self.cu[b]:self.cu[b + 1]][None], k[b:b + 1, :h + n], v[b:b + 1, :h + n]
