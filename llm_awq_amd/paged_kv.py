"""Host-side page allocator for the paged KV cache (`ops.attn_kvcache_paged`, `ops.rope_kv_store_paged`,
`QuantLlamaAttentionFused.forward(block_table=, page_size=)`).

A pool of `num_pages` pages of `page_size` tokens is shared by `max_batch` slots.  `PageTable` keeps the free list on the host and the block
table on the device: `table` is an int32 [max_batch, pages_per_seq] tensor that is only ever updated IN PLACE, so its pointer is stable and a
captured graph that reads it follows every later `reserve` / `release`.  Entry [slot, i] names the page that holds tokens
i * page_size .. (i + 1) * page_size - 1 of the slot; entries behind a slot's pages hold 0, a valid page id that the kernels never read.

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
        self._held = [[] for _ in range(self.max_batch)]

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages(self, slot: int):
        """The pages `slot` holds, in logical order."""
        return tuple(self._held[slot])

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
        self._free.extend(reversed(held))
        n = len(held)
        held.clear()
        if n:
            self.table[slot, :n].zero_()
        return n
