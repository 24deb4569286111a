"""Host-side page allocator for the paged KV cache (`ops.attn_kvcache_paged`, `ops.rope_kv_store_paged`,
`QuantLlamaAttentionFused.forward(block_table=, page_size=)`).

A pool of `num_pages` pages of `page_size` tokens is shared by `max_batch` slots.  `PageTable` keeps the free list on the host and the block
table on the device: `table` is an int32 [max_batch, pages_per_seq] tensor that is only ever updated IN PLACE, so its pointer is stable and a
captured graph that reads it follows every later `reserve` / `release`.  Entry [slot, i] names the page that holds tokens
i * page_size .. (i + 1) * page_size - 1 of the slot; entries behind a slot's pages hold 0, a valid page id that the kernels never read.
Under a sliding window (`ops.attn_varq_window`) the head of a slot dies as the sequence grows: `release_before` hands those
pages back and zeroes their entries, which the windowed kernels no longer read either.

A page may have several holders: `fork` hands the whole pages of a slot's prompt to a second slot (the same ids, written into the second
slot's row), and a page goes back to the free list when its LAST holder lets go.  `PrefixGroups` keeps the three device arrays that
`ops.attn_kvcache_paged_shared` reads -- who shares how many tokens with whom -- so that the shared pages are fetched once per group.

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
        self._refs = [0] * self.num_pages  # holders of each page (slots naming it in their row); 0: on the free list

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
        for p in new:
            self._refs[p] = 1
        first = len(held)
        held.extend(new)
        self.table[slot, first:first + more].copy_(torch.tensor(new, dtype=torch.int32))  # in place: the pointer a graph captured stays valid
        return tuple(new)

    def refcount(self, page: int) -> int:
        """How many slots hold `page` (0: it is free)."""
        return self._refs[page]

    def _drop(self, pages):
        """One holder lets go of each of `pages`; yields, in order, those nobody holds any more."""
        for p in pages:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                yield p

    def fork(self, src: int, dst: int, n_tokens: int):
        """Hand the first `n_tokens` tokens of `src` to `dst`, which must hold nothing: `dst` SHARES the n_tokens // page_size whole pages
        (the same ids, written in place into its table row, one more holder each) and, when n_tokens % page_size != 0, gets one fresh page
        for the partly filled tail.  Returns that (src_page, dst_page) pair -- the caller copies it with `ops.kv_page_copy` before `dst`
        stores a token -- or None.  New tokens of `dst` land at positions >= n_tokens: in the tail copy, then in pages of its own
        (`reserve`); a shared page is never written.  Refuses a range that holds pages `release_before` handed back."""
        n = int(n_tokens)
        if src == dst or self._held[dst]:
            raise ValueError(f"PageTable.fork: slot {dst} must hold nothing and differ from slot {src}")
        whole, tail = divmod(max(n, 0), self.page_size)
        need = whole + (1 if tail else 0)
        held = self._held[src]
        if n < 1 or need > len(held):
            raise ValueError(f"PageTable.fork: slot {src} holds {len(held)} pages, {n} tokens need {need}")
        if any(p is None for p in held[:need]):
            raise ValueError(f"PageTable.fork: slot {src} has handed back pages below token {n} (release_before)")
        if tail and not self._free:
            raise PagePoolExhausted(f"PageTable: the fork of slot {src} into {dst} needs a page for the tail, none of {self.num_pages} is free")
        row = list(held[:whole])
        for p in row:
            self._refs[p] += 1
        pair = None
        if tail:
            fresh = self._free.pop()
            self._refs[fresh] = 1
            row.append(fresh)
            pair = (held[whole], fresh)
        self._held[dst].extend(row)
        self.table[dst, :len(row)].copy_(torch.tensor(row, dtype=torch.int32))  # in place
        return pair

    def common_prefix(self, slots) -> int:
        """The tokens covered by the leading table entries that all of `slots` hold in common (whole pages; 0 for no slot)."""
        rows = [self._held[s] for s in slots]
        if not rows:
            return 0
        n = 0
        for entries in zip(*rows):
            if entries[0] is None or any(e != entries[0] for e in entries):
                break
            n += 1
        return n * self.page_size

    def release(self, slot: int):
        """Return every page of `slot` to the pool (a shared page only when `slot` was its last holder); its table row goes back to 0.
        Returns the number of pages the slot let go of."""
        held = self._held[slot]
        live = [p for p in held if p is not None]
        self._free.extend(self._drop(reversed(live)))
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
        self._free.extend(self._drop(held[i] for i in reversed(dead)))
        for i in dead:
            held[i] = None
        self.table[slot, dead[0]:dead[-1] + 1].zero_()  # in place; the entries between two dead pages are dead (and zero) already
        return len(dead)


class PrefixGroups:
    """The group arrays of `ops.attn_kvcache_paged_shared`, owned here and only ever updated IN PLACE (stable pointers: a captured graph
    follows every later `set` / `clear` / `remove`).

      group_members  int32 [num_groups, group_cap]: the slots of group g in list order, -1 padding
      group_prefix   int32 [num_groups]: the tokens group g shares (0: the group is empty)
      seq_prefix     int32 [max_batch]: the tokens slot b shares with its group (0: ungrouped)

    A slot belongs to at most one group and seq_prefix[b] always equals its group's group_prefix -- what the kernels require.  The first
    listed member that is active serves as the group's lead on the device; a finished member may simply turn inactive (length -1) and be
    `remove`d later.  max_prefix, the host bound of every prefix (a multiple of 64), is what `set` accepts at most.  With a `PageTable`
    given, `set` checks that the members really hold the pages of the prefix in common."""

    def __init__(self, num_groups: int, group_cap: int, max_batch: int, max_prefix: int, device, page_table: PageTable = None):
        if num_groups < 1 or group_cap < 1 or max_batch < 1:
            raise ValueError("PrefixGroups: num_groups, group_cap and max_batch must be positive")
        if max_prefix < 64 or max_prefix % 64:
            raise ValueError(f"PrefixGroups: max_prefix {max_prefix} must be a multiple of 64, at least 64")
        self.num_groups, self.group_cap, self.max_batch, self.max_prefix = int(num_groups), int(group_cap), int(max_batch), int(max_prefix)
        self.page_table = page_table
        self.group_members = torch.full((self.num_groups, self.group_cap), -1, dtype=torch.int32, device=device)
        self.group_prefix = torch.zeros(self.num_groups, dtype=torch.int32, device=device)
        self.seq_prefix = torch.zeros(self.max_batch, dtype=torch.int32, device=device)
        self._members = [[] for _ in range(self.num_groups)]
        self._prefix = [0] * self.num_groups
        self._group_of = {}

    def members(self, g: int):
        return tuple(self._members[g])

    def prefix(self, g: int) -> int:
        return self._prefix[g]

    def group_of(self, slot: int):
        return self._group_of.get(slot)

    def _write_row(self, g: int):
        row = self._members[g] + [-1] * (self.group_cap - len(self._members[g]))
        self.group_members[g].copy_(torch.tensor(row, dtype=torch.int32))

    def set(self, g: int, slots, n_tokens: int):
        """Group g := `slots` (list order; the first active one leads), sharing `n_tokens` tokens.  Replaces what g held."""
        slots, n = [int(s) for s in slots], int(n_tokens)
        if not slots or len(slots) > self.group_cap or len(set(slots)) != len(slots) or any(s < 0 or s >= self.max_batch for s in slots):
            raise ValueError(f"PrefixGroups.set: 1 .. {self.group_cap} distinct slots in [0, {self.max_batch}) are expected, got {slots}")
        if n < 64 or n > self.max_prefix:
            raise ValueError(f"PrefixGroups.set: {n} shared tokens; 64 .. max_prefix = {self.max_prefix} are expected")
        if any(self._group_of.get(s, g) != g for s in slots):
            raise ValueError("PrefixGroups.set: a slot belongs to one group at most")
        if self.page_table is not None and self.page_table.common_prefix(slots) < (n & ~63):
            raise ValueError(f"PrefixGroups.set: slots {slots} hold only {self.page_table.common_prefix(slots)} tokens of pages in common, "
                             f"{n} were asked for")
        self.clear(g)
        self._members[g], self._prefix[g] = slots, n
        for s in slots:
            self._group_of[s] = g
        self._write_row(g)
        self.group_prefix[g:g + 1].fill_(n)
        self.seq_prefix[torch.tensor(slots, dtype=torch.long, device=self.seq_prefix.device)] = n
        return self

    def clear(self, g: int):
        """Group g := empty; its members become ungrouped."""
        old = self._members[g]
        if old:
            self.seq_prefix[torch.tensor(old, dtype=torch.long, device=self.seq_prefix.device)] = 0
            for s in old:
                del self._group_of[s]
        self._members[g], self._prefix[g] = [], 0
        self._write_row(g)
        self.group_prefix[g:g + 1].zero_()

    def remove(self, slot: int):
        """Take `slot` out of its group (a finished sequence); the others keep their order.  Returns the group it left, or None."""
        g = self._group_of.pop(int(slot), None)
        if g is None:
            return None
        self._members[g].remove(int(slot))
        self.seq_prefix[int(slot):int(slot) + 1].zero_()
        if self._members[g]:
            self._write_row(g)
        else:
            self.clear(g)
        return g
