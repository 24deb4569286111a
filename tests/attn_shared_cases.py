"""Needle batches for shared-prefix decode on the paged KV cache (awq_attn_kvcache_paged_shared): inputs whose exact answer is known to the bit.

The construction is that of tests/attn_prefill_cases.py (code / vrow of tests/attn_cases.py): the key at position p of a slot is
code(keyid[p] + salt), a query is AMP * code(sought id + salt), the value row is vrow(uid[p], salt).  Here the members of a group hold the
SAME ids below the group's prefix (uid = position) and ids of their own behind it (uid = position + 512 * (slot + 1)); the salt belongs to
the group (or to an ungrouped slot).  With `pair`, the first key behind a member's prefix repeats the id of the last prefix key, so a query
that seeks it returns the exact mean of the two value rows -- a result that changes when either key is attended twice or not at all.
With `decoy`, the last prefix key repeats the id of the one before it: a row whose causal limit lies between the two must not see it.

What the query of (slot b, position i, head h) seeks, by gh = h % G:
    0   the last key the row attends (the diagonal; behind the prefix)
    1   the last key of the prefix (P - 1); ungrouped: the key in the middle of the row's range
    2   the first key behind the prefix (P); ungrouped: key 0
    3   a hash of (b, i, h) over the attended keys, prefix and suffix alike
The target is the mean of vrow over the attended positions that hold the sought id (one or two of them), exact in T.

The pools are scattered as in tests/attn_paged_cases.py: shuffled page ids, NaN in every pool row that holds no key, a POISON page (NaN) in
every table entry behind a slot's live range and in the padding columns of the wider row stride.  The whole pages below a group's prefix
are the same page ids in every member's row; a page the prefix ends inside (page_size 128, P = 192) is a copy per member.
`poisoned_table()` is the table of the poison test: every non-lead member's entries wholly below the prefix name the poison page.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.attn_cases import AMP, code, vrow

P = 192
MAX_PREFIX = 256  # looser than P: pfx's min() decides
PAD_COLS = 3
SPARE_PAGES = 2
CHUNKS = (64, 256)


def _salt(sid: int, kvh: int, Hkv: int) -> int:
    return (13 + 7919 * (sid * Hkv + kvh)) % 40000


class SharedBatch:
    """spec: H, Hkv, Dh, Sq, page_size, dtype, lens (Sk per slot, None = inactive), groups ((listed slots, group_prefix), ..), bound,
    offset, pair (bool), decoy (bool), cap (group_cap, >= the longest list), undefined ({chunk: slots without a defined result})."""

    def __init__(self, spec):
        self.spec = s = dict(spec)
        self.dtype = dt = s["dtype"]
        H, Hkv, Dh, Sq, ps = s["H"], s["Hkv"], s["Dh"], s["Sq"], s["page_size"]
        self.lens_spec, self.bound, self.offset = tuple(s["lens"]), s["bound"], s["offset"]
        self.ps, self.Sq, self.G = ps, Sq, H // Hkv
        G = self.G
        B = len(self.lens_spec)
        self.cap = s["cap"]
        self.max_prefix = s.get("max_prefix", MAX_PREFIX)
        self.causal, self.scale = True, None
        assert self.cap * Sq * G <= 128 and self.max_prefix <= self.bound
        # the group arrays
        self.members = [list(m) + [-1] * (self.cap - len(m)) for m, _ in s["groups"]]
        self.group_prefix = [p for _, p in s["groups"]]
        self.seq_prefix = [0] * B
        group_of = {}
        for g, (listed, p) in enumerate(s["groups"]):
            for m in listed:
                if 0 <= m < B and self.lens_spec[m] is not None and p >= 64:
                    self.seq_prefix[m] = p
                    group_of[m] = g
        self.seqlens_k = torch.tensor([-1 if n is None else n - self.offset for n in self.lens_spec], dtype=torch.int32)
        assert self.offset <= 1 or None not in self.lens_spec
        self.lens = [int(n) + self.offset for n in self.seqlens_k]  # Sk_b as the kernels form it
        self.lead = {}
        for g, (listed, p) in enumerate(s["groups"]):
            self.lead[g] = next((m for m in listed if 0 <= m < B and self.lens_spec[m] is not None), None)

        # ---- ids ----
        self.pps = pps = (self.bound + ps - 1) // ps
        uid, keyid, sid = {}, {}, {}
        for b, n in enumerate(self.lens_spec):
            if n is None:
                continue
            pb = self.seq_prefix[b]
            u = np.arange(n, dtype=np.int64)
            u[pb:] += 512 * (b + 1)
            kid = u.copy()
            if pb and s.get("decoy"):
                kid[pb - 1] = kid[pb - 2]
            if pb and s.get("pair") and n > pb:
                kid[pb] = kid[pb - 1]
            uid[b], keyid[b], sid[b] = u, kid, (100 + group_of[b]) if b in group_of else b
        # ---- pages: whole prefix pages once per group, everything else per slot ----
        need = {b: (n + ps - 1) // ps for b, n in enumerate(self.lens_spec) if n is not None}
        shared_pages = {g: p // ps for g, (_, p) in enumerate(s["groups"]) if p >= 64 and self.lead[g] is not None}
        total = sum(need.values()) - sum(shared_pages[group_of[b]] for b in group_of) + sum(shared_pages.values())
        self.num_pages = total + SPARE_PAGES + 1
        gen = torch.Generator().manual_seed(1000 * ps + 31 * B + self.bound + Sq)
        order = torch.randperm(self.num_pages, generator=gen).tolist()
        self.poison = order.pop()
        gpages = {g: [order.pop() for _ in range(k)] for g, k in shared_pages.items()}
        self.pages = {}
        for b in need:
            head = gpages[group_of[b]] if b in group_of else []
            self.pages[b] = head + [order.pop() for _ in range(need[b] - len(head))]
        assert len(order) == SPARE_PAGES
        self.table_full = torch.full((B, pps + PAD_COLS), self.poison, dtype=torch.int32)
        self.table = self.table_full[:, :pps]
        for b in need:
            self.table_full[b, :need[b]] = torch.tensor(self.pages[b], dtype=torch.int32)
        nan = float("nan")
        self.k_pool = torch.full((self.num_pages, ps, Hkv, Dh), nan, dtype=dt)
        self.v_pool = torch.full((self.num_pages, ps, Hkv, Dh), nan, dtype=dt)
        for b in need:
            n = self.lens_spec[b]
            salt = [_salt(sid[b], kvh, Hkv) for kvh in range(Hkv)]
            K = np.stack([code(keyid[b] + salt[kvh], Dh) for kvh in range(Hkv)], 1)  # [n, Hkv, Dh]
            V = np.stack([vrow(uid[b], np.full(n, salt[kvh]), Dh, False) for kvh in range(Hkv)], 1)
            Kt, Vt = torch.from_numpy(K).to(dt), torch.from_numpy(V).to(dt)
            for i, page in enumerate(self.pages[b]):
                lo, hi = i * ps, min(n, (i + 1) * ps)
                old = self.k_pool[page, :hi - lo]
                # a shared page is written by every member with the same bits
                assert torch.isnan(old).all() or torch.equal(old.view(torch.int16), Kt[lo:hi].view(torch.int16))
                self.k_pool[page, :hi - lo] = Kt[lo:hi]
                self.v_pool[page, :hi - lo] = Vt[lo:hi]
        # ---- queries and targets ----
        self.q = torch.empty(B, Sq, H, Dh, dtype=dt)
        self.target = torch.zeros(B, Sq, H, Dh, dtype=dt)
        self.has_target = torch.zeros(B, dtype=torch.bool)
        for b, n in enumerate(self.lens_spec):
            if n is None:  # only a q is needed
                self.q[b] = torch.from_numpy(AMP * code(np.arange(Sq * H).reshape(Sq, H) + 7 * b, Dh)).to(dt)
                self.has_target[b] = True  # zeros
                continue
            pb = self.seq_prefix[b]
            for i in range(Sq):
                lim = i + n - Sq
                for h in range(H):
                    kvh, gh = h // G, h % G
                    salt = _salt(sid[b], kvh, Hkv)
                    if lim < 0:  # attends nothing: zeros
                        self.q[b, i, h] = torch.from_numpy(AMP * code(np.int64(i + h), Dh)).to(dt)
                        continue
                    pos = (lim, pb - 1 if pb else lim // 2, min(pb, lim), (b * 2654435761 + i * 40503 + h * 977 + 11) % (lim + 1))[gh % 4]
                    sought = keyid[b][pos]
                    hit = np.nonzero(keyid[b][:lim + 1] == sought)[0]
                    assert 1 <= len(hit) <= 2
                    t = vrow(uid[b][hit], np.full(len(hit), salt), Dh, False).astype(np.float64).mean(0)
                    tt = torch.from_numpy(t.astype(np.float32)).to(dt)
                    assert torch.equal(tt.double(), torch.from_numpy(t))  # exact in T
                    self.q[b, i, h] = torch.from_numpy(AMP * code(sought + salt, Dh)).to(dt)
                    self.target[b, i, h] = tt
            self.has_target[b] = True
        self.undefined = {c: set(v) for c, v in s.get("undefined", {}).items()}

    def defined(self, chunk: int):
        """bool [B]: the slots whose result the contract defines under a forced chunk (and whose target is therefore binding)."""
        ok = self.has_target.clone()
        for b in self.undefined.get(chunk, ()):
            ok[b] = False
        return ok

    def poisoned_table(self):
        """The table with every non-lead member's entries WHOLLY below its prefix naming the poison page (same shape and stride)."""
        t = self.table_full.clone()
        for g, (listed, p) in enumerate(self.spec["groups"]):
            for m in listed:
                if m != self.lead[g] and 0 <= m < len(self.lens) and self.seq_prefix[m]:
                    eff = min(self.seq_prefix[m], self.max_prefix, max(0, self.lens[m] - self.Sq)) & ~63  # what the suffix walk starts at
                    t[m, :eff // self.ps] = self.poison
        return t


def _cases():
    out = []
    n = 0
    for dt in (torch.float16, torch.bfloat16):
        tag = str(dt)[6:]
        for Dh in (64, 128):
            for Sq in (1, 3):
                for ps in (64, 128):
                    # slot 0 inactive and listed first; group 0 = [0, 4, 1, 3] at lengths P + Sq, P + 70, P + 130; slot 2 a group of its own;
                    # slot 5 ungrouped; slot 6 in a group whose group_prefix is 0; group 3 lists only an inactive slot and an index outside
                    lens = (None, P + 70, P + 70, P + 130, P + Sq, 150, 100)
                    groups = (((0, 4, 1, 3), P), ((2,), P), ((6,), 0), ((0, 99), P))
                    out.append(dict(name=f"main-Dh{Dh}-Sq{Sq}-ps{ps}-{tag}", H=8, Hkv=2, Dh=Dh, Sq=Sq, page_size=ps, dtype=dt, lens=lens, groups=groups,
                                    bound=384, offset=(0, 1)[n % 2], pair=True, cap=5))
                    n += 1
        # all 128 rows of the tile: 32 members x G 4, Sq 1
        lens = tuple(P + 1 + (7 * t) % 90 for t in range(32))
        out.append(dict(name=f"full-tile-{tag}", H=8, Hkv=2, Dh=64, Sq=1, page_size=64, dtype=dt, lens=lens, groups=((tuple(range(31, -1, -1)), P),),
                        bound=320, offset=1, pair=True, cap=32))
        # group_prefix exceeds Sk - Sq of slot 1 (P + 1 keys, Sq 3: 190 < 192).  pfx clamps its own prefix to 128; under chunk 64 its two
        # prefix entries are keys [0, 128) of the lead's P_g = 192 and its suffix begins at 128 -- attn_kvcache_paged's result.  Under chunk
        # 256 the one prefix entry holds keys [0, 192), beyond its causal limit: the contract leaves slot 1 unspecified there.
        out.append(dict(name=f"short-member-{tag}", H=8, Hkv=2, Dh=128, Sq=3, page_size=64, dtype=dt, lens=(P + 40, P + 1, P + 90),
                        groups=(((2, 1, 0), P),), bound=320, offset=3, decoy=True, cap=3, undefined={256: (1,)}))
    return out


CASES = _cases()


def case_id(spec) -> str:
    return spec["name"]


_BUILT = {}


def build(spec) -> SharedBatch:
    """One SharedBatch per spec, built once and shared by the tests (never modified)."""
    if spec["name"] not in _BUILT:
        _BUILT[spec["name"]] = SharedBatch(spec)
    return _BUILT[spec["name"]]
