"""numpy restatement of the speculative-decoding contracts (include/awq_cdna4.h: awq_spec_draft_ngram / awq_spec_pack / awq_spec_verify /
awq_spec_accept; DESIGN.md "Speculative decoding"), and a toy model on which the speculative loop must emit what the token-by-token loop emits.

The row arithmetic is tests/sample_oracle.py's: `verify` calls its `sample_row` per packed row, so the margins it returns mean what they mean there.

The toy model: the logits of a position are a row of a table [V, V] chosen by the token fed at that position, and the uniform of a position comes
from a table indexed by (slot, absolute cache position).  The serial loop (one `sample_row` + step 9 per slot and step) and the speculative loop
(draft -> pack -> gather -> verify -> accept) therefore see the same logits and the same uniform at every generated position, and must agree on
tokens, history, hist_len, seqlens and finished exactly -- both are float64 computations on the same rows, so no margin is involved.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import sample_oracle as SO


# ------------------------------------------------------------------------------------------------------------------------
# the four contracts
# ------------------------------------------------------------------------------------------------------------------------
def draft_ngram(history, hist_len, seqlens, vocab, kmax, ngram_min, ngram_max, max_len, max_draft=None):
    """-> (drafts int32 [B, kmax] with -1 behind the draft, draft_len int32 [B])"""
    history = np.asarray(history)
    B, Lh = history.shape
    drafts = np.full((B, kmax), -1, np.int32)
    draft_len = np.zeros(B, np.int32)
    for b in range(B):
        L, h = int(hist_len[b]), history[b]
        if seqlens[b] < 0 or L > Lh or L < ngram_min + 1:
            continue
        best = None
        for i in range(L - 1):
            m = 0
            while m < ngram_max and i - m >= 0 and h[i - m] == h[L - 1 - m]:
                m += 1
            if m >= ngram_min and (best is None or (m, i) > best):
                best = (m, i)
        if best is None:
            continue
        i = best[1]
        md = kmax if max_draft is None else max(0, int(max_draft[b]))
        c = max(0, min(kmax, md, L - 1 - i, int(max_len) - int(seqlens[b]) - 1))
        cont = h[i + 1:i + 1 + c]
        bad = np.flatnonzero((cont < 0) | (cont >= vocab))
        if bad.size:
            c = int(bad[0])
        drafts[b, :c] = h[i + 1:i + 1 + c]
        draft_len[b] = c
    return drafts, draft_len


def pack(last_tokens, drafts, draft_len, seqlens, total_q):
    """-> (cu int32 [B + 1], input_ids int32 [total_q], drafts and draft_len as rewritten)"""
    drafts = np.array(drafts, dtype=np.int32, copy=True)
    B, kmax = drafts.shape
    act = np.asarray(seqlens) >= 0
    d = np.where(act, np.clip(np.asarray(draft_len, dtype=np.int64), 0, kmax), 0)
    R = int(total_q) - int(act.sum())
    E = np.cumsum(d) - d
    c = np.clip(R - E, 0, d)
    n = np.where(act, 1 + c, 0)
    cu = np.zeros(B + 1, np.int32)
    cu[1:] = np.cumsum(n)
    ids = np.full(total_q, -1, np.int32)
    for b in range(B):
        drafts[b, c[b]:] = -1
        if act[b]:
            ids[cu[b]] = last_tokens[b]
            ids[cu[b] + 1:cu[b] + 1 + c[b]] = drafts[b, :c[b]]
    return cu, ids, drafts, c.astype(np.int32)


def owner(cu, B, r):
    """varq_owner: the last b with cu[b] <= r, or None for r >= cu[B]"""
    if r >= cu[B]:
        return None
    return int(np.flatnonzero(np.asarray(cu[:B]) <= r)[-1])


def penalty_set(history_row, hist_len_b, ids, cu_b, j):
    """the ids the serial loop would hold in the history when it samples the burst's row j"""
    Lh = len(history_row)
    hl = int(hist_len_b)
    out = list(history_row[:min(max(hl, 0), Lh)])
    out += [int(ids[cu_b + i]) for i in range(1, j + 1) if 0 <= hl + i - 1 < Lh]
    return out


def verify(logits_f32, u, cu, ids, B, t, k, p, r, history=None, hist_len=None, mutant=None):
    """-> (row_tokens int32 [total_q], margins [total_q]); t / k / p / r are per-slot arrays; mutant: a fault of sample_oracle.MUTANTS"""
    T = logits_f32.shape[0]
    toks, margins = np.full(T, -1, np.int32), np.full(T, np.inf)
    for row in range(T):
        b = owner(cu, B, row)
        if b is None:
            continue
        j = row - int(cu[b])
        hist = penalty_set(history[b], hist_len[b], ids, int(cu[b]), j) if history is not None else ()
        toks[row], margins[row], _ = SO.sample_row(logits_f32[row], u[row], t[b], p[b], int(k[b]), r[b], hist, mutant=mutant)
    return toks, margins


def step9(tok, b, history, hist_len, seqlens, stop_ids, finished, max_len, append=True, advance=True):
    """step 9 of the sampling contract for one token of slot b, in place"""
    if append and history is not None:
        if 0 <= hist_len[b] < history.shape[1]:
            history[b, hist_len[b]] = tok
        hist_len[b] += 1
    stop = int(tok) in set(int(s) for s in stop_ids)
    if stop and finished is not None:
        finished[b] = 1
    if advance:
        seqlens[b] = -1 if (stop or seqlens[b] + 1 >= max_len) else seqlens[b] + 1


def accept(row_tokens, ids, cu, kmax, history, hist_len, seqlens, stop_ids, finished, max_len, append=True, advance=True):
    """in place on history / hist_len / seqlens / finished -> (out_tokens [B, kmax + 1], num_emitted [B], last_tokens [B])"""
    B = len(cu) - 1
    out = np.full((B, kmax + 1), -1, np.int32)
    num, last = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b in range(B):
        c0, n = int(cu[b]), min(int(cu[b + 1]) - int(cu[b]), kmax + 1)
        if n <= 0 or (seqlens is not None and seqlens[b] < 0):
            continue
        a = 0
        while a <= n - 2 and row_tokens[c0 + a] == ids[c0 + a + 1]:
            a += 1
        for j in range(a + 1):
            tok = int(row_tokens[c0 + j])
            out[b, j] = tok
            num[b] += 1
            last[b] = tok
            step9(tok, b, history, hist_len, seqlens, stop_ids, finished, max_len, append, advance)
            if advance and seqlens[b] < 0:
                break
    return out, num, last


# ------------------------------------------------------------------------------------------------------------------------
# planted drafter rows, with the drafts worked out by hand (ngram_min 1, ngram_max 3, kmax 4, vocab 100, max_len 1000, Lh 64)
# ------------------------------------------------------------------------------------------------------------------------
DRAFT_KW = dict(vocab=100, kmax=4, ngram_min=1, ngram_max=3, max_len=1000)
_TWICE = [1, 2, 3, 40, 41, 42, 43, 44, 1, 2, 3, 50, 51, 52, 53, 54, 1, 2, 3]   # (1, 2, 3) ends at 2 and at 10: the later one is continued
# (name, history, hist_len or None = len(history), seqlen, max_draft, the draft)
DRAFT_CASES = (
    ("no_match", [1, 2, 3, 4, 5, 6, 7, 8], None, 10, 4, []),
    ("older_3gram_beats_2gram", [7, 8, 9, 20, 21, 22, 23, 3, 8, 9, 30, 31, 32, 33, 7, 8, 9], None, 10, 4, [20, 21, 22, 23]),
    ("later_of_two_equal", _TWICE, None, 10, 4, [50, 51, 52, 53]),
    ("abababab", [5, 6] * 4, None, 10, 4, [5, 6]),                              # the match ends at 5; only L - 1 - i = 2 tokens follow it
    ("match_ends_at_index_0", [9, 4, 5, 6, 7, 9], None, 10, 4, [4, 5, 6, 7]),
    ("L_equals_ngram_min", [3], None, 10, 4, []),
    ("overflowed_history", ([1, 2, 3, 4] * 16), 64 + 3, 10, 4, []),
    ("inactive_slot", _TWICE, None, -1, 4, []),
    ("max_draft_0", _TWICE, None, 10, 0, []),
    ("max_len_cap", _TWICE, None, 997, 4, [50, 51]),                            # 1000 - 997 - 1 = 2 rows fit the cache behind the slot's own
    ("id_outside_vocab", [1, 2, 3, 50, 51, 100, 53, 54, 1, 2, 3], None, 10, 4, [50, 51]),
)


def draft_case_arrays(rows, Lh=64):
    """the planted rows `rows` as the drafter's arrays -> (history [n, Lh], hist_len, seqlens, max_draft, drafts [n, 4], draft_len), the last
    two by hand"""
    n, kmax = len(rows), DRAFT_KW["kmax"]
    history, hist_len = np.full((n, Lh), 77, np.int32), np.zeros(n, np.int32)
    seqlens, max_draft = np.zeros(n, np.int32), np.zeros(n, np.int32)
    drafts, draft_len = np.full((n, kmax), -1, np.int32), np.zeros(n, np.int32)
    for j, i in enumerate(rows):
        _, h, hl, seq, md, d = DRAFT_CASES[i]
        history[j, :len(h)] = h
        hist_len[j] = len(h) if hl is None else hl
        seqlens[j], max_draft[j] = seq, md
        drafts[j, :len(d)] = d
        draft_len[j] = len(d)
    return history, hist_len, seqlens, max_draft, drafts, draft_len


# ------------------------------------------------------------------------------------------------------------------------
# the toy model and the two loops
# ------------------------------------------------------------------------------------------------------------------------
TOY_V, TOY_B, TOY_LH, TOY_KMAX, TOY_STEPS, TOY_PERIOD = 257, 3, 40, 4, 40, 6
# greedy; temperature + top-k + top-p; with a repetition penalty
TOY_PARAMS = dict(t=np.array([0.0, 0.8, 0.7], np.float32), k=np.array([0, 20, 0], np.int32), p=np.array([1.0, 0.9, 1.0], np.float32),
                  r=np.array([1.0, 1.0, 1.3], np.float32))


def toy_table(seed=0, V=TOY_V, boost=7.0):
    """fp32 [V, V]: N(0, 1) with one favoured successor per token; the successors run in cycles of TOY_PERIOD, so the text repeats itself"""
    rng = np.random.default_rng(seed)
    tab = rng.standard_normal((V, V)).astype(np.float32)
    v = np.arange(V)
    succ = np.where(v % TOY_PERIOD == TOY_PERIOD - 1, v - (TOY_PERIOD - 1), v + 1)
    succ = np.where(succ >= V, v - v % TOY_PERIOD, succ)
    tab[v, succ] += np.float32(boost)
    return tab, succ


def toy_state(seed=0):
    """-> dict: table, u_tab [B, max_len + kmax + 1], the start state (history, hist_len, seqlens, finished, last_tokens), max_len, stop_ids.
    Prompts hold a cycle and a half, so the first step can draft; the shortest sequence ends at max_len after exactly TOY_STEPS serial steps;
    Lh = 40 overflows on the way for the longer prompts (the drafter then gives up, both loops go on)."""
    tab, succ = toy_table(seed)
    rng = np.random.default_rng(seed + 1)
    B, Lh = TOY_B, TOY_LH
    history = np.zeros((B, Lh), np.int32)
    hist_len = np.zeros(B, np.int32)
    last = np.zeros(B, np.int32)
    seqlens = np.array([4, 9, 14], np.int32)
    for b, start in enumerate((12, 60, 126)):
        toks = [start]
        for _ in range(seqlens[b]):
            toks.append(int(succ[toks[-1]]))
        history[b, :len(toks)] = toks       # the prompt and the token fed next (the sampler appended it when it drew it)
        hist_len[b] = len(toks)
        last[b] = toks[-1]
    max_len = int(seqlens.min()) + TOY_STEPS
    u_tab = rng.random((B, max_len + TOY_KMAX + 1)).astype(np.float32)
    return dict(table=tab, u_tab=u_tab, history=history, hist_len=hist_len, seqlens=seqlens, finished=np.zeros(B, np.int32), last_tokens=last,
                max_len=max_len, stop_ids=np.array([TOY_V - 1], np.int32))


def _copy_state(s):
    return {k: s[k].copy() for k in ("history", "hist_len", "seqlens", "finished", "last_tokens")}


def serial_loop(s, params=TOY_PARAMS, steps=TOY_STEPS):
    """one sample_row + step 9 per active slot and step -> (tokens [steps, B] with -1 for inactive slots, final state, steps until all finished)"""
    st = _copy_state(s)
    B = st["seqlens"].size
    toks = np.full((steps, B), -1, np.int32)
    done = steps
    for it in range(steps):
        for b in range(B):
            if st["seqlens"][b] < 0:
                continue
            hl = int(st["hist_len"][b])
            hist = st["history"][b, :min(hl, st["history"].shape[1])]
            tok = SO.sample_row(s["table"][st["last_tokens"][b]], s["u_tab"][b, st["seqlens"][b]], params["t"][b], params["p"][b], int(params["k"][b]),
                                params["r"][b], hist)[0]
            toks[it, b] = tok
            st["last_tokens"][b] = tok
            step9(tok, b, st["history"], st["hist_len"], st["seqlens"], s["stop_ids"], st["finished"], s["max_len"])
        if (st["seqlens"] < 0).all() and done == steps:
            done = it + 1
    return toks, st, done


def spec_inputs(s, st, cu, ids):
    """the toy model's gather: per packed row the logits (zeros for a padding row) and the uniform of its absolute position"""
    T, B = ids.size, st["seqlens"].size
    logits = np.zeros((T, s["table"].shape[1]), np.float32)
    u = np.zeros(T, np.float32)
    for row in range(T):
        b = owner(cu, B, row)
        if b is None:
            continue
        logits[row] = s["table"][ids[row]]
        u[row] = s["u_tab"][b, st["seqlens"][b] + row - cu[b]]
    return logits, u


def spec_loop(s, params=TOY_PARAMS, steps=TOY_STEPS, kmax=TOY_KMAX, ngram_min=1, ngram_max=3, total_q=None):
    """draft -> pack -> gather -> verify -> accept per step -> (out_tokens [steps, B, kmax + 1], num_emitted [steps, B], final state, steps
    until all finished)"""
    st = _copy_state(s)
    B = st["seqlens"].size
    total_q = B * (kmax + 1) if total_q is None else total_q
    outs, nums = np.full((steps, B, kmax + 1), -1, np.int32), np.zeros((steps, B), np.int32)
    done = steps
    for it in range(steps):
        drafts, dl = draft_ngram(st["history"], st["hist_len"], st["seqlens"], s["table"].shape[1], kmax, ngram_min, ngram_max, s["max_len"])
        cu, ids, _, _ = pack(st["last_tokens"], drafts, dl, st["seqlens"], total_q)
        logits, u = spec_inputs(s, st, cu, ids)
        rt, _ = verify(logits, u, cu, ids, B, params["t"], params["k"], params["p"], params["r"], st["history"], st["hist_len"])
        outs[it], nums[it], st["last_tokens"] = accept(rt, ids, cu, kmax, st["history"], st["hist_len"], st["seqlens"], s["stop_ids"], st["finished"],
                                                       s["max_len"])
        if (st["seqlens"] < 0).all() and done == steps:
            done = it + 1
    return outs, nums, st, done


def toy_state_with_stop(seed=0, slot=1, index=20):
    """toy_state whose stop id is a token that `slot` emits in the middle of its run (the one at `index` of its unstopped serial stream), so a
    slot finishes by a stop id, possibly inside an accepted burst"""
    s = toy_state(seed)
    s["stop_ids"] = np.array([TOY_V - 1, stream(serial_loop(s)[0])[slot][index]], np.int32)
    return s


def stream(tokens_per_step):
    """the emitted tokens of every slot in order, from serial tokens [steps, B] or speculative out_tokens [steps, B, kmax + 1]"""
    a = np.asarray(tokens_per_step)
    a = a[:, :, None] if a.ndim == 2 else a
    return [[int(x) for x in a[:, b].ravel() if x >= 0] for b in range(a.shape[1])]


# ------------------------------------------------------------------------------------------------------------------------
# the verifier on sample_oracle's edge rows
# ------------------------------------------------------------------------------------------------------------------------
# the grid rows a configuration's three slots bring: u = 0 alone; u = 1 - 2^-24 and one more; five inside
EDGE_BURSTS = ((SO.U_GRID,), (SO.U_GRID + 1, 3), (17, 30, 41, 52, 60))


@functools.lru_cache(maxsize=None)
def edge_verify_case(V, dtype_name):
    """Every configuration of sample_oracle.build_edge_case as three slots (bursts of 1, 2 and 5 rows) with the configuration's parameters and
    history; every row is the configuration's logits row under one of its grid uniforms.  The inputs behind a slot's first row are an id its
    history holds already (penalty slots) or any id, so the penalty set is the configuration's and the oracle's tokens are the grid's.  Three
    padding rows (NaN) behind.  -> arrays, `grid`: the grid's tokens per row, `want` / `margin`: verify's own.  Shared, never written."""
    cfgs = SO.build_edge_case(V, dtype_name)
    slots = [(ci, picks) for ci in range(len(cfgs)) for picks in EDGE_BURSTS]
    B = len(slots)
    cu = np.zeros(B + 1, np.int32)
    cu[1:] = np.cumsum([len(picks) for _, picks in slots])
    T = int(cu[-1]) + 3
    ids, u, src, grid = np.full(T, -1, np.int32), np.zeros(T, np.float32), np.zeros(T, np.int64), np.full(T, -1, np.int64)
    par = dict(t=np.ones(B, np.float32), k=np.zeros(B, np.int32), p=np.ones(B, np.float32), r=np.ones(B, np.float32),
               history=np.zeros((B, SO.HIST_LEN), np.int32), hist_len=np.zeros(B, np.int32))
    for b, (ci, picks) in enumerate(slots):
        c = cfgs[ci]
        for name in ("t", "k", "p", "r", "history", "hist_len"):
            par[name][b] = c[name]
        for j, i in enumerate(picks):
            row = cu[b] + j
            u[row], src[row], grid[row] = c["u"][i], ci, c["token"][i]
            ids[row] = (3 * b + 1) % V if j == 0 else SO.head_ids(V)[0] if c["r"] > 1 else (7 * j + b) % V
    logits = torch.stack([c["logits"] for c in cfgs])[torch.from_numpy(src)].contiguous()
    logits[cu[-1]:] = float("nan")        # padding rows are not read
    want, margin = verify(logits.float().numpy(), u, cu, ids, B, par["t"], par["k"], par["p"], par["r"], par["history"], par["hist_len"])
    return dict(case=par, cu=cu, ids=ids, u=u, logits=logits, want=want, margin=margin, grid=grid, T=T, M=B)


PEN_BURST = 5   # rows per slot of penalty_burst_case


@functools.lru_cache(maxsize=None)
def penalty_burst_case(V, dtype_name):
    """32 slots (16 on the ladder from 2.0, 16 on the one from -1.0), penalty 1.5, an EMPTY history: the penalty set of a row is the burst's
    earlier inputs alone -- nothing, then the top head id, then V + (the rank-2 head id), which the contract ignores, then the top id again, then
    the rank-1 id.  Slot s draws every row near u = (s % 16 + 0.5) / 16.  -> as edge_verify_case"""
    B = 32
    h = SO.head_ids(V)
    cu = (np.arange(B + 1) * PEN_BURST).astype(np.int32)
    T = int(cu[-1])
    ids = np.tile(np.array([(V // 2) | 1, h[0], V + h[2], h[0], h[1]], np.int32), B)
    par = dict(t=np.ones(B, np.float32), k=np.zeros(B, np.int32), p=np.ones(B, np.float32), r=np.full(B, 1.5, np.float32),
               history=np.zeros((B, SO.HIST_LEN), np.int32), hist_len=np.zeros(B, np.int32))
    xs = [SO.ladder_logits(V, 2.0), SO.ladder_logits(V, -1.0)]
    u, src = np.zeros(T, np.float32), np.repeat(np.arange(B) // 16, PEN_BURST)
    for sign in range(2):
        for j in range(PEN_BURST):
            row = SO.Row(SO.process(xs[sign], 1.0, 1.5, penalty_set(par["history"][0], 0, ids, 0, j)))
            mask = row.kept()[0]
            for s in range(16):
                u[(16 * sign + s) * PEN_BURST + j] = SO.robust_u(row, mask, np.float32((s + 0.5) / 16))
    logits = torch.from_numpy(np.stack(xs)).to(SO.TORCH_DTYPES[dtype_name])[torch.from_numpy(src)].contiguous()
    want, margin = verify(logits.float().numpy(), u, cu, ids, B, par["t"], par["k"], par["p"], par["r"], par["history"], par["hist_len"])
    return dict(case=par, cu=cu, ids=ids, u=u, logits=logits, want=want, margin=margin, T=T, M=B)
