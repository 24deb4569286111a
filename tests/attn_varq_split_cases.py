"""One MIXED packed step (awq_attn_varq[_kv8], awq_attn_paged_varq[_kv8]; csrc/awq_varq.hpp "who serves a sequence"): the split-KV pair takes
the short sequences over a long history, the one-pass kernel everything else, decided on the device by ONE rule.

    the split pair takes sequence b  iff  1 <= Sq_b <= max_seqlen_q and 1 <= Sk_b <= max_seqlen_k (active),
                                          Sq_b <= split_seqlen_q and Sk_b >= split_min_keys

STEP lists (new tokens, history before the step) so that every term of the rule decides the route of at least one sequence, under H 8 /
Hkv 2 (G = 4), max_seqlen_k 512, split_min_keys 128, split_seqlen_q 8, max_seqlen_q 70, the split chunk forced to 64:

    (1, 256)   taken; Sk 257, one key behind a chunk edge          (9, 300)   one row too many: one-pass
    (1, 127)   Sk 128, exactly the floor: taken                    (0, 500)   nothing written
    (1, 126)   Sk 127: one-pass                                    (70, 64)   a prompt chunk across a 64-row tile: one-pass
    (8, 200)   taken; several causal rows, R = 32                  (1, -1)    a slot at -1: inactive, zeros from the one-pass kernel
    (3, 509)   fills the bound exactly: taken                      (2, 511)   beyond the bound: inactive, zeros

`takes` restates the rule on the CPU; `routes` applies it to the step.  The mutants, one plausible fault each:

    floor+1        Sk_b > split_min_keys                 sq+1            Sq_b <= split_seqlen_q + 1
    floor-1        Sk_b >= split_min_keys - 1            sq-1            Sq_b <  split_seqlen_q
    before-off     lens_before_step ignored when Sk_b is formed
    inactive-taken the activity term dropped: a sequence beyond the bound is handed to the split pair

`Step` holds the tensors of the step on the CPU: packed q with PAD_ROWS rows of NaN behind cu[B], caches [B, BOUND + 7, Hkv, Dh] that hold
NaN in every row that holds no key, the lengths in either convention; `Pool` scatters the caches into shuffled pages behind a table whose
row stride is wider than pages_per_seq, NaN in every unused row and a poison page (all NaN) in every unused entry."""
from __future__ import annotations

import torch

H, HKV = 8, 2
G = H // HKV
BOUND = 512
LMAX = BOUND + 7
CHUNK = 64
SPLIT_MIN_KEYS = 128
SPLIT_SEQLEN_Q = 8
MAX_Q = 70
PAD_ROWS = 9
SENTINEL = 3.0
PAGE_SIZES = (64, 128)
PAD_COLS = 3
STEP = ((1, 256), (1, 127), (1, 126), (8, 200), (9, 300), (0, 500), (70, 64), (1, -1), (3, 509), (2, 511))
TAKEN = (True, True, False, True, False, False, False, False, True, False)   # written down by hand, not computed
MUTANTS = ("floor+1", "floor-1", "sq+1", "sq-1", "before-off", "inactive-taken")
COMBOS = [(torch.float16, 64), (torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64)]


def takes(sq, seqlen_k, before, max_q=MAX_Q, bound=BOUND, split_q=SPLIT_SEQLEN_Q, floor=SPLIT_MIN_KEYS, mutant=None):
    """The rule for one sequence: sq = cu[b + 1] - cu[b], seqlen_k = seqlens_k[b], before = lens_before_step."""
    sk = seqlen_k + (sq if before and mutant != "before-off" else 0)
    active = 1 <= sq <= max_q and 1 <= sk <= bound
    if mutant == "inactive-taken":
        active = sq >= 1
    if mutant == "floor+1":
        floor += 1
    if mutant == "floor-1":
        floor -= 1
    if mutant == "sq+1":
        split_q += 1
    if mutant == "sq-1":
        split_q -= 1
    return active and sq <= split_q and sk >= floor


def seqlens(before, step=STEP):
    """seqlens_k of the step: the histories (lens_before_step) or the totals."""
    return [h if before else h + n for n, h in step]


def routes(before=True, mutant=None, step=STEP, **kw):
    """Per sequence: True = the split pair."""
    return tuple(takes(n, s, before, mutant=mutant, **kw) for (n, _), s in zip(step, seqlens(before, step)))


def active(b, step=STEP):
    n, h = step[b]
    return 0 <= n <= MAX_Q and 1 <= h + n <= BOUND


class Step:
    """The tensors of STEP for (dtype, Dh), on the CPU.  q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N."""

    def __init__(self, dtype, Dh, step=STEP):
        self.dtype, self.Dh, self.step = dtype, Dh, step
        B = len(step)
        self.sq = [n for n, _ in step]
        self.cu = [0]
        for n in self.sq:
            self.cu.append(self.cu[-1] + n)
        self.total_q = self.cu[-1] + PAD_ROWS
        # keys the cache holds for b after the step: an active sequence's Sk_b, an idle slot's history, nothing for an inactive one
        self.held = [(h + n if active(b, step) else 0) for b, (n, h) in enumerate(step)]
        g = torch.Generator().manual_seed(977 + Dh + (1 if dtype == torch.bfloat16 else 0))
        nan = float("nan")
        self.q = torch.full((self.total_q, H, Dh), nan, dtype=dtype)
        self.q[:self.cu[-1]] = (1.5 * torch.randn(self.cu[-1], H, Dh, generator=g)).to(dtype)
        self.k_cache = torch.full((B, LMAX, HKV, Dh), nan, dtype=dtype)
        self.v_cache = torch.full((B, LMAX, HKV, Dh), nan, dtype=dtype)
        for b, n in enumerate(self.held):
            self.k_cache[b, :n] = torch.randn(n, HKV, Dh, generator=g).to(dtype)
            self.v_cache[b, :n] = (1 + 0.5 * torch.randn(n, HKV, Dh, generator=g)).to(dtype)
        self.cu_seqlens_q = torch.tensor(self.cu, dtype=torch.int32)

    def seqlens_k(self, before=True):
        return torch.tensor(seqlens(before, self.step), dtype=torch.int32)

    def offset(self, b, before=True):
        """seqlen_offset of the rectangular call on sequence b alone."""
        return self.sq[b] if before else 0


class Pool:
    """A Step's caches scattered into pages of `ps` keys: a shuffled table (no page in its identity place), the poison page in every entry
    behind a live range and in the table's padding columns, a row stride wider than pages_per_seq."""

    def __init__(self, st: Step, ps: int):
        self.ps, self.pps = ps, (BOUND + ps - 1) // ps
        B = len(st.held)
        need = [(n + ps - 1) // ps for n in st.held]
        self.num_pages = sum(need) + 3
        for attempt in range(64):
            order = torch.randperm(self.num_pages, generator=torch.Generator().manual_seed(31 * ps + st.Dh + 7919 * attempt)).tolist()
            self.poison = order.pop()
            pages = [[order.pop() for _ in range(need[b])] for b in range(B)]
            if all(page != b * self.pps + i for b in range(B) for i, page in enumerate(pages[b])):
                break
        else:
            raise AssertionError("no shuffle without a page in its identity place")
        self.table_full = torch.full((B, self.pps + PAD_COLS), self.poison, dtype=torch.int32)
        self.table = self.table_full[:, :self.pps]
        nan = float("nan")
        self.k_pool = torch.full((self.num_pages, ps, HKV, st.Dh), nan, dtype=st.dtype)
        self.v_pool = torch.full_like(self.k_pool, nan)
        for b in range(B):
            for i, page in enumerate(pages[b]):
                self.table_full[b, i] = page
                lo, hi = i * ps, min(st.held[b], (i + 1) * ps)
                self.k_pool[page, :hi - lo], self.v_pool[page, :hi - lo] = st.k_cache[b, lo:hi], st.v_cache[b, lo:hi]
        assert torch.isnan(self.k_pool[self.poison]).all() and self.table.stride(0) > self.table.shape[1]

    def gather(self, b, n):
        p = torch.arange(n)
        page = self.table[b, p // self.ps].long()
        return self.k_pool[page, p % self.ps], self.v_pool[page, p % self.ps]
