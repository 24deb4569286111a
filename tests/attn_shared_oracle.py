"""Shared-prefix decode on the paged KV cache (awq_attn_kvcache_paged_shared, csrc/awq_shared.hpp) restated in torch on the CPU.

The contract of include/awq_cdna4.h, step by step, with the per-split arithmetic of `tests.attn_splitkv_oracle.splitkv` (fp32 base-2
logits, every weight rounded to T once, unnormalised partials; the combine in ascending entry order with m = -inf skipped):

    pfx(P, Sk)   = min(P, max_prefix, max(0, Sk - Sq)) & ~63, 0 for P < 64
    prefix side  per group: lead = the first listed member that is a slot index and active; P_g = pfx(group_prefix[g], Sk_lead); prefix
                 split s = keys [s * chunk_p, min(P_g, (s + 1) * chunk_p)) read through the LEAD's table row, no mask; the partial of
                 member j's rows goes to entry s of that member's workspace rows (valid, active members only)
    suffix side  per active b: P_b = pfx(seq_prefix[b], Sk_b); suffix split s = keys [P_b + s * chunk_s, min(Sk_b, ..)) through b's own row,
                 causal mask as attn_kvcache_paged; entry splits_p + s
    combine      per b: entries 0 .. ceil(P_b / chunk_p) - 1, then splits_p .. ; zeros when nothing was attended

The workspace starts as NaN: an entry that is combined without having been written shows as NaN, as garbage would on the device.

`mutant` switches one fault in:
    noprefix      the prefix entries are not combined
    anchor-64     the suffix splits are anchored at P_b - 64: a tile of the prefix is attended twice
    anchor+64     .. at P_b + 64: the first tile behind the prefix is never attended
    memberminor   the q row of a packed prefix row is looked up member-minor, r = (i * G + gh) * group_cap + j, while it is stored member-major
    leadfirst     the lead is the first listed slot index, active or not
    prefixmask    the causal mask is applied inside the prefix, as if the sequence ended at P_g
    noclamp       pfx without the Sk - Sq term
"""
from __future__ import annotations

import torch

from tests import attn_splitkv_oracle as S

MUTANTS = ("noprefix", "anchor-64", "anchor+64", "memberminor", "leadfirst", "prefixmask", "noclamp")
NINF = float("-inf")


def pfx(P: int, max_prefix: int, Sk: int, Sq: int, mutant=None) -> int:
    room = Sk if mutant == "noclamp" else max(0, Sk - Sq)
    e = min(int(P), max_prefix, room)
    return (e & ~63) if e > 0 else 0


def plan(max_prefix: int, bound: int, chunk: int):
    """(splits_p, chunk_p, splits_s, chunk_s) under a forced chunk."""
    return (max_prefix + chunk - 1) // chunk, chunk, (bound + chunk - 1) // chunk, chunk


def _partial(Q, K, V, sc, T, lo, lim=None):
    """One split as `S.splitkv` computes it: Q [R, Dh] fp32, K / V [n, Dh] of T holding keys lo .. lo + n - 1; lim [R]: the last key a
    row attends (None: every key).  -> (O [R, Dh], m [R], l [R])."""
    f32 = torch.float32
    x = (Q @ K.to(f32).T) * sc
    if lim is not None:
        x = x.masked_fill(torch.arange(lo, lo + K.shape[0])[None, :] > lim[:, None], NINF)
    m = x.max(-1).values
    p = torch.exp2(x - torch.where(m == NINF, torch.zeros_like(m), m)[:, None]).to(T).to(f32)
    return p @ V.to(f32), m, p.sum(-1)


def shared(q, k_pool, v_pool, table, lens, bound, members, group_prefix, seq_prefix, max_prefix, chunk_p, chunk_s, scale=None, causal=True,
           mutant=None):
    """q [B, Sq, H, Dh] T, pools [num_pages, page_size, Hkv, Dh] T, table int [B, >= pages_per_seq], lens: Sk_b per slot as the kernel
    forms it (any int), members: one list of ints per group (-1 padding allowed), group_prefix / seq_prefix: ints.  -> out T."""
    B, Sq, H, Dh = q.shape
    num_pages, ps, Hkv, _ = k_pool.shape
    G, T, f32 = H // Hkv, q.dtype, torch.float32
    R = Sq * G
    sc = torch.tensor((float(Dh) ** -0.5 if scale is None else float(scale)), dtype=f32) * torch.tensor(S.LOG2E, dtype=f32)
    splits_p, splits_s = (max_prefix + chunk_p - 1) // chunk_p, (bound + chunk_s - 1) // chunk_s
    n_ent = splits_p + splits_s
    active = [1 <= n <= bound for n in lens]
    rows = torch.arange(R)
    qi, qg = rows // G, rows % G  # a member's own rows: i * G + gh
    nan = float("nan")
    ws_o = torch.full((B, Hkv, R, n_ent, Dh), nan, dtype=f32)
    ws_m = torch.full((B, Hkv, R, n_ent), nan, dtype=f32)
    ws_l = torch.full((B, Hkv, R, n_ent), nan, dtype=f32)

    def keys(b, lo, hi, kvh):
        p = torch.arange(lo, hi)
        page = table[b, p // ps].long().clamp(0, num_pages - 1)
        return k_pool[page, p % ps, kvh], v_pool[page, p % ps, kvh]

    # ---- prefix side ----
    for g, listed in enumerate(members):
        cap = len(listed)
        valid = [0 <= m < B for m in listed]
        lead = next((m for m, ok in zip(listed, valid) if ok and (active[m] or mutant == "leadfirst")), None)
        if lead is None:
            continue
        P_g = pfx(group_prefix[g], max_prefix, lens[lead], Sq, mutant)
        for s in range(splits_p):
            lo = s * chunk_p
            if lo >= P_g:
                continue
            hi = min(P_g, lo + chunk_p)
            for kvh in range(Hkv):
                K, V = keys(lead, lo, hi, kvh)
                for j, m in enumerate(listed):
                    if not (valid[j] and active[m]):
                        continue
                    if mutant == "memberminor":  # packed row r of the tile takes the q of (j', i', gh') with r = (i' * G + gh') * cap + j'
                        r = (j * Sq + qi) * G + qg
                        jj, rest = r % cap, r // cap
                        src = torch.tensor([min(max(listed[x], 0), B - 1) for x in jj.tolist()])
                        Q = q[src, rest // G, kvh * G + rest % G].to(f32)
                    else:
                        Q = q[m, qi, kvh * G + qg].to(f32)
                    lim = qi + (P_g - Sq) if mutant == "prefixmask" else None
                    O, mm, l = _partial(Q, K, V, sc, T, lo, lim)
                    ws_o[m, kvh, :, s], ws_m[m, kvh, :, s], ws_l[m, kvh, :, s] = O, mm, l

    # ---- suffix side and combine ----
    out = torch.zeros_like(q)
    for b in range(B):
        if not active[b]:
            continue
        Sk = lens[b]
        P_b = pfx(seq_prefix[b], max_prefix, Sk, Sq, mutant)
        anchor = max(0, P_b + {"anchor-64": -64, "anchor+64": 64}.get(mutant, 0))
        lim = qi + (Sk - Sq) if causal else None
        for kvh in range(Hkv):
            Q = q[b, qi, kvh * G + qg].to(f32)
            for s in range(splits_s):
                lo = anchor + s * chunk_s
                e = splits_p + s
                if lo >= Sk:
                    ws_o[b, kvh, :, e], ws_m[b, kvh, :, e], ws_l[b, kvh, :, e] = 0.0, NINF, 0.0
                    continue
                K, V = keys(b, lo, min(Sk, lo + chunk_s), kvh)
                ws_o[b, kvh, :, e], ws_m[b, kvh, :, e], ws_l[b, kvh, :, e] = _partial(Q, K, V, sc, T, lo, lim)
            own = 0 if mutant == "noprefix" else (P_b + chunk_p - 1) // chunk_p
            ent = list(range(own)) + list(range(splits_p, n_ent))
            M = ws_m[b, kvh][:, ent].max(-1).values
            acc, L = torch.zeros(R, Dh, dtype=f32), torch.zeros(R, dtype=f32)
            for e in ent:
                m = ws_m[b, kvh, :, e]
                live = m != NINF
                w = torch.exp2(m - M)
                acc = torch.where(live[:, None], w[:, None] * ws_o[b, kvh, :, e] + acc, acc)
                L = torch.where(live, w * ws_l[b, kvh, :, e] + L, L)
            res = torch.where((M == NINF)[:, None], torch.zeros(R, Dh, dtype=f32), acc * (1.0 / L)[:, None]).to(T)
            out[b, qi, kvh * G + qg] = res
    return out


def paged(q, k_pool, v_pool, table, lens, bound, chunk, scale=None, causal=True):
    """attn_kvcache_paged on the same pools and tables, through `S.splitkv` itself: the reference the shared call must equal."""
    num_pages, ps = k_pool.shape[0], k_pool.shape[1]
    out = torch.zeros_like(q)
    for b, n in enumerate(lens):
        if n < 1 or n > bound:
            continue
        p = torch.arange(n)
        page = table[b, p // ps].long().clamp(0, num_pages - 1)
        out[b] = S.splitkv(q[b:b + 1], k_pool[page, p % ps][None], v_pool[page, p % ps][None], scale, causal, chunk=chunk)[0]
    return out
