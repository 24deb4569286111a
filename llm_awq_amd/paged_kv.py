"""Host-side page allocator for the paged KV cache (`ops.attn_kvcache_paged`, `ops.rope_kv_store_paged`,
`QuantLlamaAttentionFused.forward(block_table=, page_size=)`).

A pool of `num_pages` pages of `page_size` tokens is shared by `max_batch` slots.  `PageTable` keeps the free list on the host and the block
table on the device: `table` is an int32 [max_batch, pages_per_seq] tensor that is only ever updated IN PLACE, so its pointer is stable and a
captured graph that reads it follows every later `reserve` / `release`.  Entry [slot, i] names the page that holds tokens
i * page_size .. (i + 1) * page_size - 1 of the slot; entries behind a slot's pages hold 0, a valid page id that the kernels never read.
Under a sliding window (`ops.attn_varq_window`) the head of a slot dies as the sequence grows: `release_before` hands those
pages back and zeroes their entries, which the windowed kernels no longer read either.

Host logic only: no kernel, and nothing here reads the device.
"""
from __future__ import annotations

import torch


class PagePoolExhausted(RuntimeError):
    pass


class PageTable:
    def __init__(self, num_pages: int, page_size: int, max_batch: int, pages_per_seq: int, device):
        if page_size < 64 or page_size % 64:
            raise ValueError(f"PageTable: page_size {page_size} must be a multiple of 64, at least 64 (the key tile of the attention kernel)")
        if num_pages < 1 or max_batch < 1 or pages_per_seq < 1:
            raise ValueError("PageTable: num_pages, max_batch and pages_per_seq must be positive")
        self.num_pages, self.page_size, self.max_batch, self.pages_per_seq = int(num_pages), int(page_size), int(max_batch), int(pages_per_seq)
        self.table = torch.zeros(self.max_batch, self.pages_per_seq, dtype=torch.int32, device=device)
        self._free = list(range(self.num_pages - 1, -1, -1))  # a stack: page 0 goes out first, a released page is the next one reused
        self._held = [[] for _ in range(self.max_batch)]  # logical order; None: a head page handed back by release_before

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages(self, slot: int):
        """The pages `slot` holds, in logical order (without the head pages `release_before` handed back)."""
        return tuple(p for p in self._held[slot] if p is not None)

    def reserve(self, slot: int, n_tokens: int):
        """Grow the table row of `slot` until it covers `n_tokens` tokens (never shrinks).  Returns the pages added."""
        need = (int(n_tokens) + self.page_size - 1) // self.page_size
        held = self._held[slot]
        if need > self.pages_per_seq:
            raise ValueError(f"PageTable: {n_tokens} tokens need {need} pages, a table row holds {self.pages_per_seq}")
        more = need - len(held)
        if more <= 0:
            return ()
        if more > len(self._free):
            raise PagePoolExhausted(f"PageTable: slot {slot} asked for {more} more pages ({n_tokens} tokens), {len(self._free)} of "
                                    f"{self.num_pages} are free")
        new = [self._free.pop() for _ in range(more)]
        first = len(held)
        held.extend(new)
        self.table[slot, first:first + more].copy_(torch.tensor(new, dtype=torch.int32))  # in place: the pointer a graph captured stays valid
        return tuple(new)

    def release(self, slot: int):
        """Return every page of `slot` to the pool; its table row goes back to 0."""
        held = self._held[slot]
        live = [p for p in held if p is not None]
        self._free.extend(reversed(live))
        n = len(held)
        held.clear()
        if n:
            self.table[slot, :n].zero_()
        return len(live)

    def release_before(self, slot: int, n_tokens: int):
        """Return to the pool every page of `slot` that lies WHOLLY below token `n_tokens` -- pages i with (i + 1) * page_size <= n_tokens --
        and zero their table entries in place.  The page that holds token `n_tokens` is never released.  Returns the number of pages
        handed back (pages released earlier do not count).  The slot keeps its logical positions: `reserve` goes on growing the row behind
        its last page, `release` returns what is left, `pages` lists what is still held.

        The scheduler's rule under `window_left = left`: after a step that left the slot at Sk_b keys, n_tokens = max(0, Sk_b - left) & ~63
        is safe for EVERY later step.  A later row stands at a position p >= Sk_b and attends keys >= p - left >= Sk_b - left; the windowed
        kernels read whole 64-key tiles from the tile of their first window start, so nothing below (Sk_b - left) & ~63 -- no key, no scale,
        no table entry -- is read again.  (The step itself had Sq_b new rows whose windows reach back to Sk_b - Sq_b - left: release after
        the step, not before it.)"""
        held = self._held[slot]
        upto = min(max(int(n_tokens), 0) // self.page_size, len(held))
        dead = [i for i in range(upto) if held[i] is not None]
        if not dead:
            return 0
        self._free.extend(held[i] for i in reversed(dead))
        for i in dead:
            held[i] = None
        self.table[slot, dead[0]:dead[-1] + 1].zero_()  # in place; the entries between two dead pages are dead (and zero) already
        return len(dead)
