"""Ragged needle batches for a PROMPT CHUNK over a natural-layout KV cache with per-sequence lengths on the device, dense and paged
(awq_attn_prefill_kvcache[_kv8], awq_attn_prefill_paged[_kv8]): the shapes `tests.attn_kvcache_cases.Batch` refuses (Sq * G > 128).

Row b of a batch is a B = 1 `tests.attn_prefill_cases.Case` of the batch's (H, Hkv, Dh, Sq, dtype) with a total length Sk_b = history_b + Sq
of its own: k / v go to cache[b, :Sk_b] of a [B, bound + PAD, Hkv, Dh] cache that holds NaN everywhere else, q and the targets are stacked.
    * histories 0, 31, 63, 64, 127, 191 put the totals on, just before and just after 64-key tile and page edges;
    * one slot holds -1 (a finished slot): with total lengths (offset 0) it is inactive; with seqlen_offset = Sq it is, by the contract, a
      sequence of Sq - 1 keys whose first row has a negative causal limit (zeros) -- the cache rows 0 .. Sq - 2 it attends hold keys;
    * one history takes its sequence one key beyond the bound: inactive.  Inactive sequences have all-NaN cache rows, a q of their own
      and zero targets;
    * OFFSETS alternates between "lengths before the store" (seqlens_k = history, seqlen_offset = Sq) and total lengths (offset 0);
    * SHORT is one batch of total lengths below Sq (offset 0): the first Sq - Sk_b rows of such a sequence have a negative causal limit and
      return zeros, the last Sk_b rows are a square case; FULL is one causal = 0 batch.
Every mode of Case is one-hot (or an exact mean of two rows), so a target does not depend on the q tile.

`PagedPrefill` scatters a batch into a pool of pages as `tests.attn_paged_cases.PagedBatch` does: shuffled pages, no page in its identity
place, NaN in every pool row that holds no key, the POISON page (NaN, a valid id) behind every live range and in the table padding, a table
row stride wider than pages_per_seq.

`dense(pb, mutant)` / `paged(pp, mutant)` restate the calls on the CPU: per sequence the gather, then `tests.attn_prefill_oracle.attention` in
float64, zeros for inactive sequences and negative-limit rows.  The mutants, one plausible fault each:

    len+1 / len-1   every sequence is one key longer / shorter than its entry says
    lenswap         sequence b uses the length of sequence b + 1 (cyclic)
    bound           every sequence uses max_seqlen_k in the place of its own length
    shiftmax        the causal shift is taken from the bound (max_seqlen_k - Sq) while the keys end at Sk_b
    inactive-nan    an inactive sequence is not zeroed
    identity        the table is ignored: page i of sequence b is pool page b * pages_per_seq + i
    rowswap         the table row of sequence b + 1 (cyclic) is used
    page+1          the entry index is off by one
    slot64          the row inside a page is taken modulo 64, not modulo page_size
    stride          the table row stride is assumed to be pages_per_seq
    prevpage        the page id of the previous 64-key tile is used for this one (the look-ahead off by one)
"""
from __future__ import annotations

import torch

from tests import attn_prefill_oracle as O
from tests.attn_prefill_cases import Case

H, HKV = 8, 2
SQS = (33, 65, 130)            # 33: the first size the split pair refuses; 130: two 128-row q tiles with a 2-row tail (three of 64 rows)
HISTORIES = (0, 31, 63, 64, 127, 191)
BOUND = 384
PAD = 7                        # cache rows behind the bound (NaN like every row that holds no key)
PAGE_SIZES = (64, 128)
PAD_COLS = 3                   # table columns behind pages_per_seq
SPARE_PAGES = 2                # pages nobody holds
TILE = 64
LEN_MUTANTS = ("len+1", "len-1", "lenswap", "bound", "shiftmax", "inactive-nan")
PAGE_MUTANTS = ("identity", "rowswap", "page+1", "slot64", "stride", "prevpage")
SHORT_TOTALS = (20, 64, 65, 100, 1, None)   # with Sq = 65: three sequences with negative-limit rows, one square, one longer, one slot at -1


class PrefillBatch:
    """spec["lens"]: the totals Sk_b (None: the slot at -1, whose total is seqlen_offset - 1; "over": one key beyond the bound)."""

    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        Dh, Sq = s["Dh"], s["Sq"]
        self.bound, self.offset, self.mode = s["bound"], s["offset"], s["mode"]
        self.causal = s.get("causal", True)
        self.lens = tuple(self.offset - 1 if n is None else (self.bound + 1 if n == "over" else n) for n in s["lens"])
        self.slots = tuple(b for b, n in enumerate(s["lens"]) if n is None)   # the entries that hold -1
        self.lmax = self.bound + PAD
        B = len(self.lens)
        nan = float("nan")
        self.k_cache = torch.full((B, self.lmax, HKV, Dh), nan, dtype=dt)
        self.v_cache = torch.full((B, self.lmax, HKV, Dh), nan, dtype=dt)
        self.q = torch.empty(B, Sq, H, Dh, dtype=dt)
        self.target = torch.zeros(B, Sq, H, Dh, dtype=dt)
        self.rows, self.scale = [], None
        for b, n in enumerate(self.lens):
            live = self.active(n)
            # an inactive row, and the rows of a short sequence whose limit is negative, only need a finite q: a square case's
            filler = Case(dict(B=1, H=H, Hkv=HKV, Dh=Dh, Sq=Sq, Sk=Sq + b, dtype=dt, causal=self.causal, padq=0, padk=0,
                               mode="negscale" if self.mode == "negscale" else "diag"))
            self.q[b] = filler.q[0]
            self.scale = filler.scale
            self.rows.append(None)
            if not live:
                continue
            rows = min(Sq, n) if self.causal else Sq   # causal and Sk_b < Sq: the last Sk_b rows are a square case, the others attend nothing
            row = dict(B=1, H=H, Hkv=HKV, Dh=Dh, Sq=rows, Sk=n, dtype=dt, causal=self.causal, padq=0, padk=0)
            if self.mode == "pair" and n >= 65:
                row.update(mode="pair", pair=(63, 64))
            elif self.mode == "pair":                   # too short for the pair: the diagonal
                row.update(mode="diag")
            elif self.mode == "decoy":
                row.update(mode="decoy", call=s["call"])
            else:
                row.update(mode=self.mode)
            case = Case(row)
            self.rows[b] = case
            self.q[b, Sq - rows:] = case.q[0]
            self.k_cache[b, :n] = case.k[0]
            self.v_cache[b, :n] = case.v[0]
            self.target[b, Sq - rows:] = case.target[0]
        self.seqlens_k = torch.tensor([n - self.offset for n in self.lens], dtype=torch.int32)
        assert all(self.seqlens_k[b] == -1 for b in self.slots) and list(self.lens) == self.total()

    def active(self, n):
        return 1 <= n <= self.bound

    def total(self):
        """Sk_b as the kernels form it."""
        return [int(n) + self.offset for n in self.seqlens_k]

    def live(self):
        return [(b, n) for b, n in enumerate(self.lens) if self.active(n)]


def _attend(pb: PrefillBatch, b: int, k, v, n: int, shift=None):
    """out T [Sq, H, Dh] of sequence b over keys k / v [n, Hkv, Dh]: tests.attn_prefill_oracle.attention in float64 on the rows that attend
    a key, zeros for the rows whose limit is negative.  shift (the shiftmax mutant): row i attends j <= min(i + shift, n - 1)."""
    Sq = pb.q.shape[1]
    out = torch.zeros_like(pb.q[b])
    if shift is not None:   # one row at a time: a single non-causal row attends every key it is given
        lim = [min(i + shift, n - 1) for i in range(Sq)]
        for i in range(Sq):
            if lim[i] >= 0:
                out[i] = O.attention(pb.q[b:b + 1, i:i + 1], k[None, :lim[i] + 1], v[None, :lim[i] + 1], pb.scale, False)[0, 0].to(pb.dtype)
        return out
    dead = max(Sq - n, 0) if pb.causal else 0
    out[dead:] = O.attention(pb.q[b:b + 1, dead:], k[None], v[None], pb.scale, pb.causal)[0].to(pb.dtype)
    return out


def _length(pb: PrefillBatch, b: int, mutant):
    tot = pb.total()
    B = len(tot)
    n = tot[(b + 1) % B] if mutant == "lenswap" else tot[b]
    n += {"len+1": 1, "len-1": -1}.get(mutant, 0)
    return pb.bound if mutant == "bound" else n


def dense(pb: PrefillBatch, mutant=None):
    """awq_attn_prefill_kvcache restated in torch on the CPU: out T [B, Sq, H, Dh]."""
    out = torch.zeros_like(pb.q)
    for b in range(pb.q.shape[0]):
        n = _length(pb, b, mutant)
        if n < 1 or n > pb.bound:
            if mutant == "inactive-nan":
                out[b] = float("nan")
            continue
        shift = pb.bound - pb.q.shape[1] if mutant == "shiftmax" and pb.causal else None
        out[b] = _attend(pb, b, pb.k_cache[b, :n], pb.v_cache[b, :n], n, shift)
    return out


def len_mutant_applies(pb: PrefillBatch, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    live = [n for _, n in pb.live()]
    if mutant == "len+1":         # cache row Sk_b holds NaN and the last query row attends it; at Sk_b = bound the sequence turns inactive: zeros
        return True
    if mutant == "len-1":         # the last attended key of every row is lost: seen where it is the target
        return pb.mode in ("diag", "negscale")
    if mutant == "lenswap":       # a longer neighbour brings NaN rows in, an inactive one zeroes; every batch here has both
        return len(set(pb.lens)) > 1 and (any(not pb.active(n) for n in pb.lens) or any(live[(i + 1) % len(live)] > n for i, n in enumerate(live)))
    if mutant == "bound":         # rows Sk_b .. bound - 1 of the cache hold NaN and the last query row attends them
        return any(n < pb.bound for n in live)
    if mutant == "shiftmax":      # a sequence shorter than the bound attends its first masked key: seen where a decoy sits there
        return pb.causal and any(c is not None and c.mode == "decoy" and c.decoys > 0 and n < pb.bound for c, n in zip(pb.rows, pb.lens))
    if mutant == "inactive-nan":
        return any(not pb.active(n) for n in pb.lens)
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# the same batches over a pool of pages
# ------------------------------------------------------------------------------------------------------------------------
class PagedPrefill:
    def __init__(self, spec):
        self.spec = dict(spec)
        self.batch = pb = PrefillBatch({k: v for k, v in spec.items() if k != "page_size"})
        self.ps = ps = spec["page_size"]
        B = len(pb.lens)
        self.pps = pps = (pb.bound + ps - 1) // ps
        need = [(n + ps - 1) // ps if pb.active(n) else 0 for n in pb.lens]
        self.num_pages = sum(need) + SPARE_PAGES + 1
        for attempt in range(64):  # (deterministic: the first shuffle that leaves no page where a table-less kernel would look)
            g = torch.Generator().manual_seed(1000 * ps + B + pb.q.shape[1] + 7919 * attempt)
            order = torch.randperm(self.num_pages, generator=g).tolist()
            self.poison = order.pop()
            self.pages = [[order.pop() for _ in range(need[b])] for b in range(B)]
            if all(page != b * pps + i for b in range(B) for i, page in enumerate(self.pages[b])):
                break
        else:
            raise AssertionError("no shuffle without a page in its identity place")
        assert len(order) == SPARE_PAGES
        self.table_full = torch.full((B, pps + PAD_COLS), self.poison, dtype=torch.int32)
        self.table = self.table_full[:, :pps]   # the row stride stays wider than pages_per_seq
        for b in range(B):
            self.table_full[b, :need[b]] = torch.tensor(self.pages[b], dtype=torch.int32)
        nan = float("nan")
        self.k_pool = torch.full((self.num_pages, ps, HKV, pb.k_cache.shape[3]), nan, dtype=pb.dtype)
        self.v_pool = torch.full_like(self.k_pool, nan)
        for b, n in pb.live():
            for i, page in enumerate(self.pages[b]):
                lo, hi = i * ps, min(n, (i + 1) * ps)
                self.k_pool[page, :hi - lo] = pb.k_cache[b, lo:hi]
                self.v_pool[page, :hi - lo] = pb.v_cache[b, lo:hi]
        # the gather through the table is the dense cache, bit for bit; everything else of the pool is NaN
        held = torch.zeros(self.num_pages, ps, dtype=torch.bool)
        for b, n in pb.live():
            k, v = gather(self, b, n)
            assert torch.equal(k.view(torch.int16), pb.k_cache[b, :n].view(torch.int16))
            assert torch.equal(v.view(torch.int16), pb.v_cache[b, :n].view(torch.int16))
            p = torch.arange(n)
            held[self.table[b, p // ps].long(), p % ps] = True
        assert not torch.isnan(self.k_pool[held]).any() and torch.isnan(self.k_pool[~held]).all() and torch.isnan(self.v_pool[~held]).all()
        assert (self.table_full[:, pps:] == self.poison).all() and all((self.table[b, need[b]:] == self.poison).all() for b in range(B))

    def dense(self):
        """(k, v) [B, pages_per_seq * page_size, Hkv, Dh]: the gather of every table row, poison pages included (NaN)."""
        idx = self.table.long()
        return tuple(t[idx].reshape(idx.shape[0], self.pps * self.ps, *t.shape[2:]) for t in (self.k_pool, self.v_pool))


def _address(pp: PagedPrefill, b: int, p: torch.Tensor, mutant=None):
    """(page, row) of logical keys p of sequence b, as the kernel forms them (page ids clamped into the pool)."""
    ps, pps = pp.ps, pp.pps
    B = pp.table.shape[0]
    idx = p // ps
    row = p % (64 if mutant == "slot64" else ps)
    if mutant == "prevpage":
        idx = (p // TILE - 1).clamp_min(0) * TILE // ps
    if mutant == "page+1":
        idx = idx + 1
    if mutant == "identity":
        page = b * pps + idx
    elif mutant == "stride":
        page = pp.table_full.reshape(-1)[b * pps + idx]
    elif mutant == "rowswap":
        page = pp.table_full[(b + 1) % B, idx]
    else:
        page = pp.table_full[b, idx]
    return page.long().clamp(0, pp.num_pages - 1), row


def gather(pp: PagedPrefill, b: int, n: int, mutant=None):
    page, row = _address(pp, b, torch.arange(n), mutant)
    return pp.k_pool[page, row], pp.v_pool[page, row]


def paged(pp: PagedPrefill, mutant=None, pools=None):
    """awq_attn_prefill_paged restated in torch on the CPU: out T [B, Sq, H, Dh].  pools: (k_pool, v_pool) to gather from in the place of
    the batch's own (the dequantised FP8 pools)."""
    pb = pp.batch
    out = torch.zeros_like(pb.q)
    for b, n in enumerate(pb.total()):
        if n < 1 or n > pb.bound:
            continue
        if pools is None:
            k, v = gather(pp, b, n, mutant)
        else:
            page, row = _address(pp, b, torch.arange(n))
            k, v = pools[0][page, row], pools[1][page, row]
        out[b] = _attend(pb, b, k, v, n)
    return out


def page_mutant_applies(pp: PagedPrefill, mutant: str) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    pb, ps = pp.batch, pp.ps
    live = pb.live()
    last_key_shows = pb.mode in ("diag", "negscale")  # the last query row's target is key Sk_b - 1
    if mutant == "identity":    # the shuffle leaves no page in its identity place (asserted above): other keys, or NaN
        return True
    if mutant == "rowswap":     # another sequence's keys carry another salt; an inactive neighbour's row is all poison
        return True
    if mutant == "page+1":      # the entry behind a sequence's last page is the poison page: NaN
        return True
    if mutant == "slot64":      # rows 64 .. page_size - 1 of a page are read from rows 0 .. : seen where the last key lives there
        return ps > 64 and last_key_shows and any((n - 1) % ps >= 64 for _, n in live)
    if mutant == "stride":      # row b >= 1 begins PAD_COLS * b entries later than assumed: a padding entry (poison) or another page
        return any(b >= 1 for b, _ in live)
    if mutant == "prevpage":    # the last key lies in a tile whose page is not the previous tile's
        return last_key_shows and any((n - 1) // TILE >= 1 and ((n - 1) // TILE * TILE) // ps != (((n - 1) // TILE - 1) * TILE) // ps
                                      for _, n in live)
    raise ValueError(mutant)


def _cases():
    out = []

    def add(name, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    n = 0
    for si, Sq in enumerate(SQS):
        lens = tuple(h + Sq for h in HISTORIES) + (None, "over")
        modes = [("diag", None), ("scatter", None), ("edges", None), ("negscale", None), ("pair", None)] + [("decoy", c) for c in range(3)]
        for mode, call in modes:
            Dh = (64, 128)[(n + si) % 2]                    # the head dims take turns, staggered so that every Sq meets both in every mode pair
            offset = (Sq, 0)[(n // 2) % 2]                  # "lengths before the store" and total lengths take turns too
            tag = mode if call is None else f"{mode}{call}"
            add(f"{tag}-Sq{Sq}-Dh{Dh}-off{offset}", Dh=Dh, Sq=Sq, lens=lens, bound=BOUND, offset=offset, mode=mode, call=call)
            n += 1
    for Dh in (64, 128):
        add(f"short-Sq65-Dh{Dh}", Dh=Dh, Sq=65, lens=SHORT_TOTALS, bound=BOUND, offset=0, mode="diag", call=None)
        add(f"full-Sq65-Dh{Dh}", Dh=Dh, Sq=65, lens=tuple(h + 65 for h in HISTORIES) + (30, None, "over"), bound=BOUND, offset=0, mode="scatter",
            call=None, causal=False)
    return out


CASES = _cases()
PAGED_CASES = [dict(s, name=f"{s['name']}-ps{ps}", page_size=ps) for s in CASES for ps in PAGE_SIZES]


def case_id(spec) -> str:
    return spec["name"]
