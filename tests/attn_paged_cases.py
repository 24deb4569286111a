"""Ragged needle batches over a PAGED KV cache (awq_attn_kvcache_paged, awq_rope_kv_store_paged_pos).

Every batch of `tests.attn_kvcache_cases` (its SHAPES, its modes, both dtypes) is scattered into a pool of pages, once per page size:

    * sequence b gets ceil(Sk_b / page_size) pages, handed out in a shuffled order, so no sequence's pages are consecutive;
    * the table row stride is wider than pages_per_seq: `table` is a view [B, pages_per_seq] of `table_full` [B, pages_per_seq + PAD_COLS],
      and the padding columns hold the id of the POISON page;
    * every pool row that holds no key -- unused pages, the tail of a sequence's last page behind Sk_b, the poison page -- is NaN;
    * every table entry behind a sequence's live range names the poison page (a valid id: reading it is harmless, attending it is not);
    * SHARED is one more batch in which sequences 0 and 1 (the same length, hence the same keys) share their first page.

`PagedBatch` asserts that the gather through the table reproduces Batch.k_cache[b, :Sk_b] / v_cache[b, :Sk_b] bit for bit.

`paged(pb, chunk, mutant)` restates the call on the CPU: per sequence the gather (with the mutant's addressing) followed by
`tests.attn_splitkv_oracle.splitkv`.  `stored(pb, new_k, new_v, pos, mutant)` restates the store.  The mutants, one plausible fault each:

    identity    the table is ignored: page i of sequence b is pool page b * pages_per_seq + i
    rowswap     the table row of sequence b + 1 (cyclic) is used
    page+1      the entry index is off by one
    slot64      the row inside a page is taken modulo 64, not modulo page_size
    stride      the table row stride is assumed to be pages_per_seq
    firstpage   one lookup per split, reused for all its tiles
    pos-page    store side: the page is taken from cache_seqlens[b] for the whole chunk
"""
from __future__ import annotations

import torch

from tests import attn_kvcache_cases as K
from tests import attn_splitkv_oracle as S

PAGE_SIZES = (64, 128)
CHUNKS = (64, 256)
PAD_COLS = 3      # table columns behind pages_per_seq
SPARE_PAGES = 2   # pages nobody holds
MUTANTS = ("identity", "rowswap", "page+1", "slot64", "stride", "firstpage")
STORE_MUTANTS = ("pos-page",)
SHARED = dict(name="shared-first-page", H=8, Hkv=2, Dh=128, Sq=1, lens=(129, 129, 65), bound=257, offset=0, mode="diag", call=None)


def _cases():
    out = []
    for spec in K.CASES:
        for ps in PAGE_SIZES:
            out.append(dict(spec, name=f"{spec['name']}-ps{ps}", page_size=ps, share=False))
    for dt in (torch.float16, torch.bfloat16):
        for ps in PAGE_SIZES:
            out.append(dict(SHARED, name=f"{SHARED['name']}-{str(dt)[6:]}-ps{ps}", dtype=dt, page_size=ps, share=True))
    return out


CASES = _cases()


def case_id(spec) -> str:
    return spec["name"]


class PagedBatch:
    def __init__(self, spec):
        self.spec = dict(spec)
        self.batch = batch = K.Batch({k: v for k, v in spec.items() if k not in ("page_size", "share")})
        self.ps = ps = spec["page_size"]
        self.share = spec["share"]
        B = len(batch.lens)
        self.pps = pps = (batch.bound + ps - 1) // ps
        need = [0 if n is None else (n + ps - 1) // ps for n in batch.lens]
        total = sum(need) - (1 if self.share else 0)
        self.num_pages = total + SPARE_PAGES + 1
        for attempt in range(64):  # (deterministic: the first shuffle that leaves no page where a table-less kernel would look)
            g = torch.Generator().manual_seed(1000 * ps + B + batch.bound + 7919 * attempt)
            order = torch.randperm(self.num_pages, generator=g).tolist()
            self.poison = order.pop()
            self.pages = []
            for b in range(B):
                mine = [order.pop() for _ in range(need[b])]
                if self.share and b == 1:
                    order.append(mine[0])   # handed back: sequence 1 reads sequence 0's first page
                    mine[0] = self.pages[0][0]
                self.pages.append(mine)
            if all(page != b * pps + i for b in range(B) for i, page in enumerate(self.pages[b])):
                break
        else:
            raise AssertionError("no shuffle without a page in its identity place")
        assert len(order) == SPARE_PAGES and len({p for m in self.pages for p in m} | {self.poison} | set(order)) == self.num_pages
        self.table_full = torch.full((B, pps + PAD_COLS), self.poison, dtype=torch.int32)
        self.table = self.table_full[:, :pps]
        for b in range(B):
            self.table_full[b, :need[b]] = torch.tensor(self.pages[b], dtype=torch.int32)
        nan = float("nan")
        Hkv, Dh = batch.k_cache.shape[2], batch.k_cache.shape[3]
        self.k_pool = torch.full((self.num_pages, ps, Hkv, Dh), nan, dtype=batch.dtype)
        self.v_pool = torch.full((self.num_pages, ps, Hkv, Dh), nan, dtype=batch.dtype)
        for b, n in enumerate(batch.lens):
            for i, page in enumerate(self.pages[b]):
                lo, hi = i * ps, min(n, (i + 1) * ps)
                self.k_pool[page, :hi - lo] = batch.k_cache[b, lo:hi]
                self.v_pool[page, :hi - lo] = batch.v_cache[b, lo:hi]
        # the gather through the table is the dense cache, bit for bit; everything else of the pool is NaN
        live = torch.zeros(self.num_pages, ps, dtype=torch.bool)
        for b, n in enumerate(batch.lens):
            if n is None:
                continue
            k, v = gather(self, b, n)
            assert torch.equal(k.view(torch.int16), batch.k_cache[b, :n].view(torch.int16))
            assert torch.equal(v.view(torch.int16), batch.v_cache[b, :n].view(torch.int16))
            p = torch.arange(n)
            live[self.table[b, p // ps].long(), p % ps] = True
        assert not torch.isnan(self.k_pool[live]).any() and torch.isnan(self.k_pool[~live]).all() and torch.isnan(self.v_pool[~live]).all()
        assert (self.table_full[:, pps:] == self.poison).all()
        for b in range(B):
            assert (self.table[b, need[b]:] == self.poison).all()

    def dense(self):
        """(k, v) [B, pages_per_seq * page_size, Hkv, Dh]: the gather of every table row, poison pages included (NaN)."""
        idx = self.table.long()
        B = idx.shape[0]
        return tuple(t[idx].reshape(B, self.pps * self.ps, *t.shape[2:]) for t in (self.k_pool, self.v_pool))


def _address(pb: PagedBatch, b: int, p: torch.Tensor, chunk: int = 64, mutant=None):
    """(page, row) of logical keys p of sequence b, as the kernel forms them (page ids clamped into the pool)."""
    ps, pps = pb.ps, pb.pps
    B = pb.table.shape[0]
    idx = p // ps
    row = p % (64 if mutant == "slot64" else ps)
    if mutant == "firstpage":
        idx = (p // chunk * chunk) // ps
    if mutant == "page+1":
        idx = idx + 1
    if mutant == "identity":
        page = b * pps + idx
    elif mutant == "stride":
        page = pb.table_full.reshape(-1)[b * pps + idx]
    elif mutant == "rowswap":
        page = pb.table_full[(b + 1) % B, idx]
    else:
        page = pb.table_full[b, idx]
    return page.long().clamp(0, pb.num_pages - 1), row


def gather(pb: PagedBatch, b: int, n: int, chunk: int = 64, mutant=None):
    page, row = _address(pb, b, torch.arange(n), chunk, mutant)
    return pb.k_pool[page, row], pb.v_pool[page, row]


def paged(pb: PagedBatch, chunk: int = 64, mutant=None):
    """The paged call restated in torch on the CPU: out T [B, Sq, H, Dh]."""
    batch = pb.batch
    out = torch.zeros_like(batch.q)
    for b, n in enumerate(batch.total()):
        if n < 1 or n > batch.bound:
            continue
        k, v = gather(pb, b, n, chunk, mutant)
        out[b] = S.splitkv(batch.q[b:b + 1], k[None], v[None], batch.scale, batch.causal, chunk=chunk)[0]
    return out


def mutant_applies(pb: PagedBatch, mutant: str, chunk: int = 64) -> bool:
    """Whether the construction is bound to see the fault (reasons, not measurements)."""
    batch, ps = pb.batch, pb.ps
    live = [(b, n) for b, n in enumerate(batch.lens) if n is not None]
    last_key_shows = batch.mode in ("diag", "negscale")  # the last query row's target is key Sk_b - 1
    if mutant == "identity":    # the shuffle leaves no page in its identity place (asserted above): other keys, or NaN
        return True
    if mutant == "rowswap":     # another sequence's keys carry another salt; an inactive neighbour's row is all poison
        return len(batch.lens) > 1
    if mutant == "page+1":      # the entry behind a sequence's last page is the poison page: NaN
        return True
    if mutant == "slot64":      # rows 64 .. page_size - 1 of a page are read from rows 0 .. : seen where the last key lives there
        return ps > 64 and last_key_shows and any((n - 1) % ps >= 64 for _, n in live)
    if mutant == "stride":      # row b >= 1 begins PAD_COLS * b entries later than assumed: a padding entry (poison) or another page
        return any(b >= 1 for b, _ in live)
    if mutant == "firstpage":   # the last key lies in a later page than its split's first key
        return last_key_shows and any(((n - 1) // chunk * chunk) // ps != (n - 1) // ps for _, n in live)
    raise ValueError(mutant)


# ------------------------------------------------------------------------------------------------------------------------
# the store restated: token s of sequence b goes to logical position pos[b] + s
# ------------------------------------------------------------------------------------------------------------------------
def stored(pb: PagedBatch, k_pool, v_pool, new_k, new_v, pos, mutant=None):
    """Writes new_k / new_v [B, S, Hkv, Dh] into clones of the pools; an inactive sequence (pos < 0 or pos + S beyond the table row) writes
    nothing.  Returns (k_pool, v_pool)."""
    k_pool, v_pool = k_pool.clone(), v_pool.clone()
    S_ = new_k.shape[1]
    for b, p0 in enumerate(pos):
        if p0 < 0 or p0 + S_ > pb.pps * pb.ps:
            continue
        p = p0 + torch.arange(S_)
        page, row = _address(pb, b, p)
        if mutant == "pos-page":
            page = _address(pb, b, torch.full((S_,), p0))[0]
        k_pool[page, row] = new_k[b]
        v_pool[page, row] = new_v[b]
    return k_pool, v_pool


def store_mutant_applies(pb: PagedBatch, pos, S_: int, mutant: str) -> bool:
    if mutant == "pos-page":    # seen only where a chunk crosses a page edge
        return any(0 <= p0 and p0 + S_ <= pb.pps * pb.ps and p0 // pb.ps != (p0 + S_ - 1) // pb.ps for p0 in pos)
    raise ValueError(mutant)
