"""Needle batches for a PACKED step of continuous batching: per-sequence query lengths on the KV-cache path, dense and paged
(awq_attn_prefill_kvcache_varq[_kv8], awq_attn_prefill_paged_varq[_kv8], awq_rope_kv_store_natural_varq[_fp8],
awq_rope_kv_store_paged_varq[_fp8]).

Sequence b of a batch brings Sq_b new tokens -- rows cu[b] .. cu[b + 1] - 1 of the packed q -- and is a B = 1
`tests.attn_prefill_cases.Case` of (H 8, Hkv 2, Dh, Sq_b, dtype) with a total length Sk_b of its own, built as
`tests.attn_prefill_kvcache_cases.PrefillBatch` builds its rows: k / v go to cache[b, :Sk_b] of a [B, BOUND + PAD, Hkv, Dh] cache that holds
NaN everywhere else.  Behind the last sequence the packed tensors carry PAD_ROWS rows of NaN: the padding of a fixed token budget.  `expect`
is what the output buffer must hold after the call when it was filled with SENTINEL before: the targets in the rows of active sequences,
zeros where the contract says zeros, SENTINEL in every row that must not be written.

    MIXED    Sq_b = (1, 33, 0, 64, 65, 130, 1, 17) over histories (191, 0, 64, 31, 63, 127, a slot at -1, one key beyond the bound),
             max_seqlen_q = 130, lengths taken before the step.  The slot at -1 with one token is a sequence of 0 keys: inactive.
    LOOSE    MIXED under max_seqlen_q = 256: whole ranks of empty blocks, the same targets.
    OVER     one sequence longer than max_seqlen_q: inactive, its first max_seqlen_q rows are zeros, the rest keep the sentinel.
    SHORT    total lengths (lens_before_step clear) with Sk_b < Sq_b for three sequences: negative-limit rows are zeros.
    FULL     one causal = 0 batch.
    UNIFORM  every Sq_b = 65: the reference is the rectangular call.

`PagedVarq` scatters a batch into a pool of pages as `tests.attn_prefill_kvcache_cases.PagedPrefill` does (shuffled pages, none in its
identity place, NaN in every row that holds no key, the POISON page behind every live range and in the table padding, a table row stride
wider than pages_per_seq) and has the attributes `gather` of that module reads.

`attend(vb, mutant, pp, pools)` restates the attention call on the CPU: per sequence slice, gather, then `tests.attn_prefill_oracle.attention`
in float64, with zeros where the contract says so.  `store_map(vb, mutant)` restates where the store launch puts every packed token.  The
mutants, one plausible fault each:

    row+1         a sequence's rows start at cu[b] + 1
    sqswap        the causal shift is formed with the neighbour's Sq (b + 1, cyclic)
    shiftmax      the causal shift is formed with max_seqlen_q
    hosttiles     the causal tile reversal counts from the host's tile count ceil(max_seqlen_q / rows), not the sequence's own
    zero-as-one   a zero-length slot is served as one row
    padding       the padding rows are written (zeros)
    inactive-skip an inactive sequence is not zeroed
    before-off    lens_before_step is ignored: Sk_b = seqlens_k[b]
    pos-t         (store) token t goes to position cache_seqlens[b] + t instead of + t - cu[b]
    tie-first     (store) a tie at a zero-length sequence goes to the FIRST sequence that begins at the token, not to its owner
"""
from __future__ import annotations

import torch

from tests import attn_prefill_kvcache_cases as K
from tests import attn_prefill_oracle as O
from tests.attn_prefill_cases import Case

H, HKV = K.H, K.HKV
BOUND = K.BOUND
PAD = K.PAD
PAGE_SIZES = K.PAGE_SIZES
PAD_COLS = K.PAD_COLS
SPARE_PAGES = K.SPARE_PAGES
PAD_ROWS = 5
SENTINEL = 3.0
MIXED_SQ = (1, 33, 0, 64, 65, 130, 1, 17)
MIXED_HIST = (191, 0, 64, 31, 63, 127, None, "over")   # None: the slot at -1; "over": Sk_b = BOUND + 1
ATTN_MUTANTS = ("row+1", "sqswap", "shiftmax", "hosttiles", "zero-as-one", "padding", "inactive-skip", "before-off")
STORE_MUTANTS = ("pos-t", "tie-first")


class VarqBatch:
    """spec: sq (Sq_b), hist (history: the keys in the cache before the step; None the slot at -1; "over" one key beyond the bound) or
    totals (Sk_b, with before = False), max_q, before, mode, Dh, dtype, causal."""

    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        Dh = s["Dh"]
        self.sq = tuple(s["sq"])
        self.max_q, self.before, self.mode, self.bound = s["max_q"], s["before"], s["mode"], BOUND
        self.causal = s.get("causal", True)
        B = len(self.sq)
        if self.before:
            self.hist = tuple(-1 if h is None else (BOUND + 1 - n if h == "over" else h) for h, n in zip(s["hist"], self.sq))
            self.lens = tuple(h + n for h, n in zip(self.hist, self.sq))
            self.seqlens_k = torch.tensor(self.hist, dtype=torch.int32)
        else:
            self.lens = tuple(-1 if n is None else (BOUND + 1 if n == "over" else n) for n in s["totals"])
            self.hist = tuple(n - q for n, q in zip(self.lens, self.sq))
            self.seqlens_k = torch.tensor(self.lens, dtype=torch.int32)
        self.cu = [0]
        for n in self.sq:
            self.cu.append(self.cu[-1] + n)
        self.total_q = self.cu[-1] + PAD_ROWS
        self.cu_seqlens_q = torch.tensor(self.cu, dtype=torch.int32)
        self.lmax = BOUND + PAD
        nan = float("nan")
        self.k_cache = torch.full((B, self.lmax, HKV, Dh), nan, dtype=dt)
        self.v_cache = torch.full((B, self.lmax, HKV, Dh), nan, dtype=dt)
        self.q = torch.full((self.total_q, H, Dh), nan, dtype=dt)
        self.expect = torch.full((self.total_q, H, Dh), SENTINEL, dtype=dt)
        self.scale = -(float(Dh) ** -0.5) if self.mode == "negscale" else None
        self.rows = []
        for b, (nq, n) in enumerate(zip(self.sq, self.lens)):
            c0 = self.cu[b]
            self.rows.append(None)
            if nq > 0:  # a finite q of its own for every row, attended or not
                filler = Case(dict(B=1, H=H, Hkv=HKV, Dh=Dh, Sq=nq, Sk=nq + b, dtype=dt, causal=self.causal, padq=0, padk=0,
                                   mode="negscale" if self.mode == "negscale" else "diag"))
                self.q[c0:c0 + nq] = filler.q[0]
            if nq == 0 and self.holds_keys(b):  # an idle slot keeps its history in the cache: nothing of it may be touched
                held = self.hist[b]
                keys = Case(dict(B=1, H=H, Hkv=HKV, Dh=Dh, Sq=1, Sk=held, dtype=dt, padq=0, padk=0, mode="diag"))
                self.k_cache[b, :held], self.v_cache[b, :held] = keys.k[0], keys.v[0]
            if not self.active(b):
                self.expect[c0:c0 + min(nq, self.max_q)] = 0   # (Sq_b = 0: no row)
                continue
            if nq == 0:
                continue
            rows = min(nq, n) if self.causal else nq   # causal and Sk_b < Sq_b: the last Sk_b rows are a square case, the others attend nothing
            row = dict(B=1, H=H, Hkv=HKV, Dh=Dh, Sq=rows, Sk=n, dtype=dt, causal=self.causal, padq=0, padk=0)
            if self.mode == "pair" and n >= 65:
                row.update(mode="pair", pair=(63, 64))
            elif self.mode == "pair":
                row.update(mode="diag")
            elif self.mode == "decoy":
                row.update(mode="decoy", call=s["call"])
            else:
                row.update(mode=self.mode)
            case = Case(row)
            self.rows[b] = case
            self.q[c0 + nq - rows:c0 + nq] = case.q[0]
            self.k_cache[b, :n], self.v_cache[b, :n] = case.k[0], case.v[0]
            self.expect[c0:c0 + nq - rows] = 0
            self.expect[c0 + nq - rows:c0 + nq] = case.target[0]

    def active(self, b):
        """The attention contract's ACTIVE: 0 <= Sq_b <= max_seqlen_q and 1 <= Sk_b <= max_seqlen_k."""
        return 0 <= self.sq[b] <= self.max_q and 1 <= self.lens[b] <= self.bound

    def holds_keys(self, b):
        """Whether the sequence owns cache rows (and pages): an active one, or an idle slot with a history."""
        n = self.lens[b] if self.sq[b] > 0 else self.hist[b]
        return 0 <= self.sq[b] <= self.max_q and 1 <= n <= self.bound

    def held(self, b):
        """Keys the cache holds for sequence b after the step."""
        if not self.holds_keys(b):
            return 0
        return self.lens[b] if self.sq[b] > 0 else self.hist[b]

    def total(self, before=None):
        """Sk_b as the kernel forms it."""
        before = self.before if before is None else before
        return [int(n) + (q if before else 0) for n, q in zip(self.seqlens_k, self.sq)]


class PagedVarq:
    """K.PagedPrefill's scattering of a VarqBatch; `gather` / `_address` of that module read ps, pps, table, table_full, num_pages, pools."""

    def __init__(self, spec):
        self.spec = dict(spec)
        self.batch = vb = VarqBatch({k: v for k, v in spec.items() if k != "page_size"})
        self.ps = ps = spec["page_size"]
        B = len(vb.sq)
        self.pps = pps = (vb.bound + ps - 1) // ps
        need = [(vb.held(b) + ps - 1) // ps for b in range(B)]
        self.num_pages = sum(need) + SPARE_PAGES + 1
        for attempt in range(64):
            g = torch.Generator().manual_seed(1000 * ps + B + vb.total_q + 7919 * attempt)
            order = torch.randperm(self.num_pages, generator=g).tolist()
            self.poison = order.pop()
            self.pages = [[order.pop() for _ in range(need[b])] for b in range(B)]
            if all(page != b * pps + i for b in range(B) for i, page in enumerate(self.pages[b])):
                break
        else:
            raise AssertionError("no shuffle without a page in its identity place")
        self.table_full = torch.full((B, pps + PAD_COLS), self.poison, dtype=torch.int32)
        self.table = self.table_full[:, :pps]
        for b in range(B):
            self.table_full[b, :need[b]] = torch.tensor(self.pages[b], dtype=torch.int32)
        nan = float("nan")
        self.k_pool = torch.full((self.num_pages, ps, HKV, vb.k_cache.shape[3]), nan, dtype=vb.dtype)
        self.v_pool = torch.full_like(self.k_pool, nan)
        held = torch.zeros(self.num_pages, ps, dtype=torch.bool)
        for b in range(B):
            n = vb.held(b)
            for i, page in enumerate(self.pages[b]):
                lo, hi = i * ps, min(n, (i + 1) * ps)
                self.k_pool[page, :hi - lo], self.v_pool[page, :hi - lo] = vb.k_cache[b, lo:hi], vb.v_cache[b, lo:hi]
            if n:
                k, v = K.gather(self, b, n)
                assert torch.equal(k.view(torch.int16), vb.k_cache[b, :n].view(torch.int16))
                assert torch.equal(v.view(torch.int16), vb.v_cache[b, :n].view(torch.int16))
                p = torch.arange(n)
                held[self.table[b, p // ps].long(), p % ps] = True
        assert not torch.isnan(self.k_pool[held]).any() and torch.isnan(self.k_pool[~held]).all() and torch.isnan(self.v_pool[~held]).all()
        assert (self.table_full[:, pps:] == self.poison).all() and all((self.table[b, need[b]:] == self.poison).all() for b in range(B))


def _keys(vb: VarqBatch, b: int, n: int, pp, pools):
    if pp is None:
        return vb.k_cache[b, :n], vb.v_cache[b, :n]
    if pools is None:
        return K.gather(pp, b, n)
    page, row = K._address(pp, b, torch.arange(n))
    return pools[0][page, row], pools[1][page, row]


def _rows(vb: VarqBatch, q, k, v, nq: int, n: int, shift: int):
    """[nq, H, Dh] in T: row s attends keys j <= min(s + shift, n - 1) (causal) or every key; zeros where the limit is negative."""
    out = torch.zeros(nq, H, q.shape[2], dtype=vb.dtype)
    if not vb.causal:
        return O.attention(q[None], k[None], v[None], vb.scale, False)[0].to(vb.dtype)
    if shift == n - nq:   # the contract's own shift: one causal call on the rows that attend a key
        dead = min(max(nq - n, 0), nq)
        if dead < nq:
            out[dead:] = O.attention(q[None, dead:], k[None], v[None], vb.scale, True)[0].to(vb.dtype)
        return out
    for s in range(nq):   # a mutant's shift: one row at a time
        lim = min(s + shift, n - 1)
        if lim >= 0:
            out[s] = O.attention(q[None, s:s + 1], k[None, :lim + 1], v[None, :lim + 1], vb.scale, False)[0, 0].to(vb.dtype)
    return out


def attend(vb: VarqBatch, mutant=None, pp=None, pools=None, tile=64):
    """The packed attention call restated on the CPU: what a buffer [total_q, H, Dh] filled with SENTINEL holds afterwards."""
    out = torch.full_like(vb.expect, SENTINEL)
    B, T = len(vb.sq), vb.total_q
    tot = vb.total(False if mutant == "before-off" else None)
    late = []
    for b in range(B):
        c0, nq, n = vb.cu[b], vb.sq[b], tot[b]
        if mutant == "row+1":
            c0 += 1
        if nq == 0 and mutant == "zero-as-one":
            late.append(b)
            continue
        if nq <= 0:
            continue
        rows = min(nq, vb.max_q)
        if not (nq <= vb.max_q and 1 <= n <= vb.bound):
            if mutant != "inactive-skip":
                out[c0:c0 + rows] = 0
            continue
        shift = n - nq
        if vb.causal and mutant == "sqswap":
            shift = n - vb.sq[(b + 1) % B]
        if vb.causal and mutant == "shiftmax":
            shift = n - vb.max_q
        k, v = _keys(vb, b, n, pp, pools)
        res = _rows(vb, vb.q[c0:c0 + nq], k, v, nq, n, shift)
        written = torch.ones(nq, dtype=torch.bool)
        if vb.causal and mutant == "hosttiles":   # rank r < ntiles_b runs tile host - 1 - r: the first host - ntiles_b tiles are never run
            host, mine = (vb.max_q + tile - 1) // tile, (nq + tile - 1) // tile
            written[:min((host - mine) * tile, nq)] = False
        out[c0:c0 + nq][written] = res[written]
    for b in late:   # the slot's one row lands on the row its successor (or the padding) owns: a race; here it wins
        c0, n = vb.cu[b], tot[b] + (1 if vb.before else 0)
        if 1 <= n <= vb.bound and c0 < T:
            k, v = _keys(vb, b, n, pp, pools)
            out[c0] = _rows(vb, vb.q[c0:c0 + 1].nan_to_num(0.0), k, v, 1, n, n - 1)[0]
        elif c0 < T:
            out[c0] = 0
    if mutant == "padding":
        out[vb.cu[-1]:] = 0
    return out


def store_map(vb: VarqBatch, mutant=None):
    """The packed store restated on the CPU: for every packed row t the (sequence, position) it is stored at, None for a row that
    stores nothing (padding, or a token of an inactive sequence -- whose q_out row is zeros); the owner is found as the kernel finds it,
    by a search over cu_seqlens_q."""
    cu, B = vb.cu, len(vb.sq)
    hist = [int(n) for n in vb.seqlens_k] if vb.before else list(vb.hist)
    out = []
    for t in range(vb.total_q):
        if t >= cu[B]:
            out.append(None)
            continue
        if mutant == "tie-first":
            b = cu.index(max(c for c in cu[:B] if c <= t))   # the first of the sequences that begin there: a zero-length one, if any
        else:
            lo, hi = 0, B   # cu[lo] <= t < cu[hi]: the LAST sequence that begins at or before t
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if cu[mid] <= t:
                    lo = mid
                else:
                    hi = mid
            b = lo
        nq = cu[b + 1] - cu[b]
        s = t - cu[b]
        if hist[b] < 0 or nq > vb.max_q or hist[b] + nq > vb.bound or not (0 <= s < nq):
            out.append(None)
            continue
        out.append((b, hist[b] + (t if mutant == "pos-t" else s)))
    return out


def store_expect(vb: VarqBatch):
    """The same map written down per sequence, without a search."""
    out = [None] * vb.total_q
    hist = [int(n) for n in vb.seqlens_k] if vb.before else list(vb.hist)
    for b, nq in enumerate(vb.sq):
        if hist[b] < 0 or nq > vb.max_q or hist[b] + nq > vb.bound:
            continue
        for s in range(nq):
            out[vb.cu[b] + s] = (b, hist[b] + s)
    return out


def _cases():
    out = []

    def add(name, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    modes = [("diag", None), ("scatter", None), ("edges", None), ("negscale", None), ("pair", None)] + [("decoy", c) for c in range(3)]
    for i, (mode, call) in enumerate(modes):
        tag = mode if call is None else f"{mode}{call}"
        add(f"mixed-{tag}-Dh{(64, 128)[i % 2]}", Dh=(64, 128)[i % 2], sq=MIXED_SQ, hist=MIXED_HIST, max_q=130, before=True, mode=mode, call=call)
    for i, (mode, call) in enumerate((("diag", None), ("decoy", 1))):
        add(f"loose-{mode}-Dh{(128, 64)[i]}", Dh=(128, 64)[i], sq=MIXED_SQ, hist=MIXED_HIST, max_q=256, before=True, mode=mode, call=call)
    for Dh, mode in ((64, "diag"), (128, "scatter")):
        add(f"over-{mode}-Dh{Dh}", Dh=Dh, sq=(40, 70, 0, 64), hist=(10, 30, 5, 64), max_q=64, before=True, mode=mode, call=None)
        add(f"short-Dh{Dh}", Dh=Dh, sq=(65, 65, 65, 33, 1, 17), totals=(20, 64, 1, 100, 50, None), max_q=65, before=False, mode="diag", call=None)
        add(f"full-Dh{Dh}", Dh=Dh, sq=(1, 33, 0, 65, 130, 17), totals=(192, 33, 64, 128, 257, "over"), max_q=130, before=False, mode="scatter",
            call=None, causal=False)
    for Dh, mode, call in ((128, "diag", None), (64, "decoy", 0)):
        add(f"uniform-{mode}-Dh{Dh}", Dh=Dh, sq=(65,) * 8, hist=K.HISTORIES + (None, "over"), max_q=65, before=True, mode=mode, call=call)
    return out


CASES = _cases()
PAGED_CASES = [dict(s, name=f"{s['name']}-ps{ps}", page_size=ps) for s in CASES for ps in PAGE_SIZES]


def case_id(spec) -> str:
    return spec["name"]


def store_mutant_applies(vb: VarqBatch, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    stored = [b for b, e in enumerate(zip(vb.sq, vb.hist)) if e[0] > 0 and e[1] >= 0 and e[0] <= vb.max_q and e[0] + e[1] <= vb.bound]
    if mutant == "pos-t":          # a stored sequence that does not begin at row 0 moves by cu[b]
        return any(vb.cu[b] > 0 for b in stored)
    if mutant == "tie-first":      # a zero-length sequence directly in front of a stored one takes its first token
        return any(vb.sq[b] == 0 and b + 1 in stored for b in range(len(vb.sq) - 1))
    raise ValueError(mutant)


def attn_mutant_applies(vb: VarqBatch, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    B = len(vb.sq)
    live = [b for b in range(B) if vb.active(b) and vb.sq[b] > 0]
    last_key_shows = vb.mode in ("diag", "negscale")
    if mutant == "row+1":          # the first row of every sequence is left unwritten
        return any(n > 0 for n in vb.sq)
    if mutant == "sqswap":         # a longer neighbour takes the diagonal away; a shorter one lets a row attend its decoy
        nxt = [vb.sq[(b + 1) % B] for b in range(B)]
        return vb.causal and ((last_key_shows and any(nxt[b] > vb.sq[b] for b in live)) or
                              (vb.mode == "decoy" and any(nxt[b] < vb.sq[b] and vb.rows[b].decoys > 0 for b in live)))
    if mutant == "shiftmax":       # a sequence shorter than the bound loses its diagonal
        return vb.causal and last_key_shows and any(vb.sq[b] < vb.max_q for b in live)
    if mutant == "hosttiles":      # a sequence with fewer 64-row tiles than the host's count loses its first tiles
        return vb.causal and any((vb.sq[b] + 63) // 64 < (vb.max_q + 63) // 64 for b in live)
    if mutant == "zero-as-one":    # the slot's row lands on a row that expects something else (a target, or the sentinel of the padding)
        return any(n == 0 for n in vb.sq)
    if mutant == "padding":
        return True
    if mutant == "inactive-skip":
        return any(not vb.active(b) and vb.sq[b] > 0 for b in range(B))
    if mutant == "before-off":     # Sk_b shrinks by Sq_b: the diagonal is lost, or a sequence without a history turns inactive
        return vb.before and ((last_key_shows and bool(live)) or any(vb.hist[b] == 0 for b in live))
    raise ValueError(mutant)
