"""not-gpu: the speculative-decoding contracts on the host -- the numpy oracle (tests/spec_oracle.py) against hand-worked drafter rows, its pack
formula against a slot-by-slot reference, the oracle's speculative loop against its serial loop on the toy model, and the argument checks of the
four C entries, which need no launch."""
import ctypes

import numpy as np
import pytest

from llm_awq_amd import _capi
from tests import sample_oracle as SO
from tests import spec_oracle as S


def test_drafter_oracle_on_hand_worked_rows():
    rows = list(range(len(S.DRAFT_CASES)))
    history, hist_len, seqlens, max_draft, want, want_len = S.draft_case_arrays(rows)
    drafts, draft_len = S.draft_ngram(history, hist_len, seqlens, max_draft=max_draft, **S.DRAFT_KW)
    for i in rows:
        assert draft_len[i] == want_len[i] and np.array_equal(drafts[i], want[i]), S.DRAFT_CASES[i][0]
    # max_draft NULL = kmax; a longer ngram_min turns the 1-token match at index 0 off
    assert np.array_equal(S.draft_ngram(history, hist_len, seqlens, **S.DRAFT_KW)[1][[2, 8]], [4, 4])
    kw = dict(S.DRAFT_KW, ngram_min=2)
    assert S.draft_ngram(history, hist_len, seqlens, **kw)[1][4] == 0 and S.draft_ngram(history, hist_len, seqlens, **kw)[1][1] == 4


def test_pack_formula_equals_the_slot_by_slot_grant():
    rng = np.random.default_rng(0)
    for trial in range(200):
        B, kmax = int(rng.integers(1, 40)), int(rng.integers(0, 16))
        seqlens = np.where(rng.random(B) < 0.25, -1, rng.integers(0, 50, B)).astype(np.int32)
        draft_len = rng.integers(-1, kmax + 3, B).astype(np.int32)   # (outside [0, kmax] now and then: clamped)
        drafts = rng.integers(0, 1000, (B, kmax)).astype(np.int32)
        last = rng.integers(0, 1000, B).astype(np.int32)
        total_q = B + int(rng.integers(0, B * (kmax + 1) + 3))
        cu, ids, new_drafts, new_len = S.pack(last, drafts, draft_len, seqlens, total_q)
        left = total_q - int((seqlens >= 0).sum())   # the rows behind the active slots' own
        want_ids, want_cu = [], [0]
        for b in range(B):
            if seqlens[b] >= 0:
                d = max(0, min(int(draft_len[b]), kmax))
                c = max(0, min(left, d))
                left -= d   # the drafts ASKED for count against the budget: once it ran out inside a slot, nobody behind gets rows
                want_ids += [int(last[b])] + drafts[b, :c].tolist()
                assert new_len[b] == c and (new_drafts[b, c:] == -1).all() and np.array_equal(new_drafts[b, :c], drafts[b, :c])
            else:
                assert new_len[b] == 0 and (new_drafts[b] == -1).all()
            want_cu.append(len(want_ids))
        assert cu.tolist() == want_cu and cu[-1] <= total_q
        assert ids.tolist() == want_ids + [-1] * (total_q - len(want_ids))


def test_oracle_verify_and_accept_on_hand_worked_bursts():
    # slot 0 brings 3 rows, slot 1 is inactive, slot 2 brings 1 row; 6 rows of budget, one padding row
    cu = np.array([0, 3, 3, 4], np.int32)
    ids = np.array([4, 1, 2, 9, -1, -1], np.int32)
    assert [S.owner(cu, 3, r) for r in range(6)] == [0, 0, 0, 2, None, None]
    # the penalty set of slot 0's rows: the history and the earlier inputs that still fit it (Lh = 4, hist_len = 3: one more fits)
    hist = np.array([[7, 8, 4, 0]], np.int32)
    assert S.penalty_set(hist[0], 3, ids, 0, 0) == [7, 8, 4] and S.penalty_set(hist[0], 3, ids, 0, 1) == [7, 8, 4, 1]
    assert S.penalty_set(hist[0], 3, ids, 0, 2) == [7, 8, 4, 1] and S.penalty_set(hist[0], 4, ids, 0, 2) == [7, 8, 4, 0]
    # accept: samples 1, 5, 6 against drafts 1, 2 -> the first draft stands, the second does not: two tokens, the second the sample itself
    state = dict(history=np.zeros((3, 8), np.int32), hist_len=np.array([2, 0, 7], np.int32), seqlens=np.array([10, -1, 20], np.int32),
                 finished=np.zeros(3, np.int32))
    out, num, last = S.accept(np.array([1, 5, 6, 3, -1, -1], np.int32), ids, cu, 2, state["history"], state["hist_len"], state["seqlens"], [99],
                              state["finished"], 100)
    assert out.tolist() == [[1, 5, -1], [-1, -1, -1], [3, -1, -1]] and num.tolist() == [2, 0, 1] and last.tolist() == [5, -1, 3]
    assert state["seqlens"].tolist() == [12, -1, 21] and state["hist_len"].tolist() == [4, 0, 8]
    assert state["history"][0, :4].tolist() == [0, 0, 1, 5] and state["history"][2, 7] == 3
    # every draft stands: the bonus token; a stop id in the middle ends the burst there
    out, num, last = S.accept(np.array([1, 2, 6, 3, -1, -1], np.int32), ids, cu, 2, state["history"], state["hist_len"], state["seqlens"], [99],
                              state["finished"], 100)
    assert out[0].tolist() == [1, 2, 6] and num[0] == 3 and state["seqlens"][0] == 15
    out, num, last = S.accept(np.array([1, 2, 6, 3, -1, -1], np.int32), ids, cu, 2, state["history"], state["hist_len"], state["seqlens"], [2],
                              state["finished"], 100)
    assert out[0].tolist() == [1, 2, -1] and num[0] == 2 and state["seqlens"][0] == -1 and state["finished"].tolist() == [1, 0, 0]


@pytest.mark.parametrize("V,dtype_name", SO.EDGE_SHAPES)
def test_the_verifier_case_on_the_edge_rows_keeps_the_grid_tokens(V, dtype_name):
    """three slots per edge configuration (1, 2 and 5 rows): the burst's inputs add nothing to a penalty set, so `verify` gives the tokens the
    sampler's grid gives, every row with the margin"""
    c = S.edge_verify_case(V, dtype_name)
    live = np.arange(c["T"]) < c["cu"][-1]
    assert sorted(set(np.diff(c["cu"]).tolist())) == [1, 2, 5] and c["M"] == 3 * len(SO.build_edge_case(V, dtype_name))
    assert (c["margin"][live] >= SO.MARGIN).all() and np.array_equal(c["want"][live], c["grid"][live]) and (c["want"][~live] == -1).all()


@pytest.mark.parametrize("V,dtype_name", [(1025, "fp32"), (1025, "bf16")])
def test_the_penalty_burst_sees_wrapped_and_repeated_inputs(V, dtype_name):
    """the burst whose earlier inputs ARE the penalty set (the history is empty): V + (a head id) entering at row 2 changes tokens under pen_wrap,
    the top id entering a second time at row 3 changes tokens under pen_per_occurrence -- with the margin on both sides"""
    c = S.penalty_burst_case(V, dtype_name)
    par = c["case"]
    h = SO.head_ids(V)
    assert S.penalty_set(par["history"][0], 0, c["ids"], 0, 1) == [h[0]] and S.penalty_set(par["history"][0], 0, c["ids"], 0, 3) == [h[0], V + h[2], h[0]]
    assert (c["margin"] >= SO.MARGIN).all()

    def kills(mutant):
        tok, margin = S.verify(c["logits"].float().numpy(), c["u"], c["cu"], c["ids"], c["M"], par["t"], par["k"], par["p"], par["r"], par["history"],
                               par["hist_len"], mutant=mutant)
        k = (tok != c["want"]) & (margin >= SO.MARGIN)
        return [int(k[j::S.PEN_BURST].sum()) for j in range(S.PEN_BURST)]

    wrap, rep = kills("pen_wrap"), kills("pen_per_occurrence")
    assert wrap[:2] == [0, 0] and wrap[2] >= 3, wrap
    assert rep[:3] == [0, 0, 0] and rep[3] >= 3, rep
    assert kills("pen_always_div")[1] >= 3           # (the ladder from -1.0: its head is negative)


@pytest.mark.parametrize("seed", range(20))
def test_oracle_speculative_loop_equals_the_serial_loop(seed):
    s = S.toy_state(seed) if seed % 2 == 0 else S.toy_state_with_stop(seed)
    toks, st, _ = S.serial_loop(s)
    out, num, st2, _ = S.spec_loop(s)
    assert S.stream(out) == S.stream(toks)
    for k in ("history", "hist_len", "seqlens", "finished"):
        assert np.array_equal(st[k], st2[k]), k
    assert (st["seqlens"] == -1).all()
    assert np.array_equal(num, (out >= 0).sum(-1))
    if seed % 2:
        assert st["finished"].any()


@pytest.mark.parametrize("make", [S.toy_state, S.toy_state_with_stop])
def test_the_toy_cases_of_the_gpu_tests_accept_drafts(make):
    """the cases tests/test_gpu_spec.py runs (seed 0): more tokens than steps for every slot, fewer steps than the serial loop, and both a rejected
    draft and a fully accepted burst occur -- the device equivalence test cannot pass with nothing ever accepted"""
    s = make(0)
    toks, _, serial_steps = S.serial_loop(s)
    out, num, _, spec_steps = S.spec_loop(s)
    assert spec_steps < serial_steps
    took = (num > 0).sum(0)
    assert (num.sum(0) > took).all(), (num.sum(0), took)
    assert (num == S.TOY_KMAX + 1).any() and ((num >= 1) & (num < S.TOY_KMAX + 1)).any()
    # a smaller token budget still agrees with the serial loop, with fewer rows per step
    out2, _, _, _ = S.spec_loop(s, total_q=S.TOY_B + 3)
    assert S.stream(out2) == S.stream(toks)


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    SHAPE, ALIGN, NULL, DTYPE = -4, -5, -6, -3

    def draft(B=2, Lh=8, V=100, kmax=4, nmin=1, nmax=3, max_len=10, **ptrs):
        a = {n: p for n in ("history", "hist_len", "seqlens", "max_draft", "drafts", "draft_len")}
        a.update(ptrs)
        return L.awq_spec_draft_ngram(a["history"], a["hist_len"], a["seqlens"], a["max_draft"], a["drafts"], a["draft_len"], B, Lh, V, kmax, nmin, nmax,
                                      max_len, None)

    for n in ("history", "hist_len", "seqlens", "drafts", "draft_len"):
        assert draft(**{n: None}) == NULL, n
    for kw in (dict(B=0), dict(Lh=0), dict(V=0), dict(kmax=-1), dict(kmax=16), dict(nmin=0), dict(nmin=4), dict(nmax=9)):
        assert draft(**kw) == SHAPE, kw
    for n in ("history", "hist_len", "seqlens", "max_draft", "drafts", "draft_len"):
        assert draft(**{n: p + 2}) == ALIGN, n

    def pack(B=2, kmax=4, total_q=10, **ptrs):
        a = {n: p for n in ("last_tokens", "drafts", "draft_len", "seqlens", "cu", "input_ids")}
        a.update(ptrs)
        return L.awq_spec_pack(a["last_tokens"], a["drafts"], a["draft_len"], a["seqlens"], a["cu"], a["input_ids"], B, kmax, total_q, None)

    for n in ("last_tokens", "drafts", "draft_len", "seqlens", "cu", "input_ids"):
        assert pack(**{n: None}) == NULL, n
        assert pack(**{n: p + 2}) == ALIGN, n
    for kw in (dict(B=0), dict(B=65536, total_q=70000), dict(kmax=-1), dict(kmax=16), dict(total_q=1)):
        assert pack(**kw) == SHAPE, kw

    vnames = ("logits", "u", "cu", "input_ids", "temperature", "top_k", "top_p", "penalty", "history", "hist_len", "row_tokens")

    def verify(dt=1, T=6, V=100, B=2, Lh=4, **ptrs):
        a = {n: p for n in vnames}
        a.update(ptrs)
        return L.awq_spec_verify(a["logits"], dt, T, V, a["u"], a["cu"], a["input_ids"], B, a["temperature"], a["top_k"], a["top_p"], a["penalty"],
                                 a["history"], a["hist_len"], Lh, a["row_tokens"], None)

    for n in ("logits", "u", "cu", "input_ids", "row_tokens", "history", "hist_len"):   # (a history comes with its lengths)
        assert verify(**{n: None}) == NULL, n
    assert verify(dt=3) == DTYPE and verify(dt=-1) == DTYPE
    for kw in (dict(T=0), dict(V=0), dict(V=(1 << 20) + 1), dict(B=0), dict(B=65536), dict(Lh=0)):
        assert verify(**kw) == SHAPE, kw
    assert verify(logits=p + 1) == ALIGN and verify(dt=2, logits=p + 2) == ALIGN
    for n in vnames[1:]:
        assert verify(**{n: p + 2}) == ALIGN, n

    anames = ("row_tokens", "input_ids", "cu", "history", "hist_len", "seqlens", "stop_ids", "finished", "out_tokens", "num_emitted", "last_tokens")

    def accept(B=2, T=6, kmax=4, Lh=4, S_=1, max_len=10, flags=3, **ptrs):
        a = {n: p for n in anames}
        a.update(ptrs)
        return L.awq_spec_accept(a["row_tokens"], a["input_ids"], a["cu"], B, T, kmax, a["history"], a["hist_len"], Lh, a["seqlens"], a["stop_ids"], S_,
                                 a["finished"], max_len, flags, a["out_tokens"], a["num_emitted"], a["last_tokens"], None)

    for n in ("row_tokens", "input_ids", "cu", "out_tokens", "num_emitted", "last_tokens", "history", "hist_len"):
        assert accept(**{n: None}) == NULL, n
    assert accept(history=None, hist_len=None, flags=1) == NULL and accept(seqlens=None, flags=2) == NULL and accept(stop_ids=None) == NULL
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(kmax=-1), dict(kmax=16), dict(Lh=0), dict(S_=-1), dict(flags=4)):
        assert accept(**kw) == SHAPE, kw
    for n in anames:
        assert accept(**{n: p + 2}) == ALIGN, n


def test_ops_and_the_sampler_class_refuse_what_they_cannot_run():
    import torch

    from llm_awq_amd import ops
    from llm_awq_amd.speculative import LM_HEAD_MAX_ROWS, PromptLookupSampler
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(_capi.AwqNativeError):
        ops.spec_draft_ngram(i32(2, 8), i32(2), i32(2), vocab=10, kmax=2)
    with pytest.raises(_capi.AwqNativeError):
        ops.spec_pack(i32(2), i32(2, 2), i32(2), i32(2), 4)
    with pytest.raises(_capi.AwqNativeError):
        ops.spec_verify(torch.zeros(4, 10), torch.zeros(4), i32(3), i32(4))
    with pytest.raises(_capi.AwqNativeError):
        ops.spec_accept(i32(4), i32(4), i32(3), 2)
    assert LM_HEAD_MAX_ROWS == 64

    class FakeSampler:   # the class checks its arguments before it touches the GPU
        batch, vocab, max_len, history = 20, 100, 50, i32(20, 8)
    with pytest.raises(ValueError, match="64 rows"):
        PromptLookupSampler(FakeSampler, i32(20), kmax=4)                       # 20 * 5 = 100 rows
    with pytest.raises(ValueError, match="at least the batch"):
        PromptLookupSampler(FakeSampler, i32(20), kmax=4, total_q=19)
    with pytest.raises(ValueError, match="kmax"):
        PromptLookupSampler(FakeSampler, i32(20), kmax=16)
    spec = PromptLookupSampler(FakeSampler, i32(20), kmax=4, allow_chunked_lm_head=True)
    assert spec.max_seqlen_q == 5 and spec.total_q == 100 and spec.lm_head_chunks() == [(0, 64), (64, 100)]
