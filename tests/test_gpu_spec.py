"""gpu: prompt-lookup speculative decoding on the device (awq_spec_draft_ngram / awq_spec_pack / awq_spec_verify / awq_spec_accept, their ops and
engine wrappers, PromptLookupSampler) against the numpy oracle of the four contracts (tests/spec_oracle.py), against `ops.sample_logits` -- the
verifier is the same row routine, so equal bits give equal tokens with no margin -- and as a loop: on a toy model the speculative loop must emit
exactly what the token-by-token `sample_logits` loop emits, in fewer steps, eagerly and replayed from one captured graph.

Rows that are compared with the ORACLE are built with sample_oracle's place_p / place_u, so every one keeps the margin derived there (asserted)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from llm_awq_amd.sampling import DeviceSampler
from llm_awq_amd.speculative import PromptLookupSampler
from tests import sample_oracle as SO
from tests import spec_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, MARK = 64, 123456789


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _np(t):
    return t.cpu().numpy()


def _guarded(*shape):
    """an int32 tensor of `shape` in the middle of a marked buffer -> (view, check): check() asserts the bands either side are untouched"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int32, device=DEV)

    def check():
        assert (flat[:GUARD] == MARK).all() and (flat[GUARD + n:] == MARK).all()
    return flat[GUARD:GUARD + n].view(*shape), check


# ------------------------------------------------------------------------------------------------------------------------
# the drafter
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [list(range(8)), [8, 9, 10, 0, 1, 2, 3, 4]], ids=["rows0-7", "rows8-10"])
def test_drafter_on_the_planted_rows(rows):
    """B = 8, Lh = 64: the eleven planted rows in two launches (the second filled up with rows of the first)"""
    history, hist_len, seqlens, max_draft, want, want_len = S.draft_case_arrays(rows)
    o_drafts, o_len = S.draft_ngram(history, hist_len, seqlens, max_draft=max_draft, **S.DRAFT_KW)
    assert np.array_equal(o_drafts, want) and np.array_equal(o_len, want_len)     # oracle = the drafts worked out by hand
    drafts, check_d = _guarded(8, 4)
    draft_len, check_l = _guarded(8)
    ops.spec_draft_ngram(_dev(history), _dev(hist_len), _dev(seqlens), max_draft=_dev(max_draft), drafts=drafts, draft_len=draft_len, **S.DRAFT_KW)
    names = [S.DRAFT_CASES[i][0] for i in rows]
    assert np.array_equal(_np(draft_len), want_len), (names, _np(draft_len), want_len)
    assert np.array_equal(_np(drafts), want), (names, _np(drafts))
    check_d(), check_l()
    # max_draft NULL = kmax
    d2, l2 = ops.spec_draft_ngram(_dev(history), _dev(hist_len), _dev(seqlens), **S.DRAFT_KW)
    o2, ol2 = S.draft_ngram(history, hist_len, seqlens, **S.DRAFT_KW)
    assert np.array_equal(_np(d2), o2) and np.array_equal(_np(l2), ol2)


@pytest.mark.parametrize("Lh", [8192, 1])
def test_drafter_one_row_at_the_ends_of_the_history_size(Lh):
    rng = np.random.default_rng(Lh)
    kw = dict(vocab=50, kmax=15, ngram_min=2, ngram_max=8, max_len=10 ** 6)
    history = rng.integers(0, 50, (1, Lh)).astype(np.int32)
    if Lh > 1:
        history[0, 3000:3012] = np.arange(20, 32)          # an 8-gram (capped) far back, 2-grams of chance everywhere after it
        history[0, Lh - 8:] = np.arange(20, 28)
    for hl in sorted({Lh, max(Lh - 5, 0), 1}):
        hist_len, seqlens = np.array([hl], np.int32), np.array([7], np.int32)
        want, want_len = S.draft_ngram(history, hist_len, seqlens, **kw)
        drafts, check_d = _guarded(1, 15)
        draft_len, check_l = _guarded(1)
        ops.spec_draft_ngram(_dev(history), _dev(hist_len), _dev(seqlens), drafts=drafts, draft_len=draft_len, **kw)
        assert np.array_equal(_np(draft_len), want_len) and np.array_equal(_np(drafts), want), (hl, _np(drafts), want)
        check_d(), check_l()
        if Lh > 1 and hl == Lh:
            assert want_len[0] == 15 and want[0, :4].tolist() == [28, 29, 30, 31]   # the capped 8-gram ends at 3007: 28 .. 31 and what follows


# ------------------------------------------------------------------------------------------------------------------------
# the packer
# ------------------------------------------------------------------------------------------------------------------------
def _pack_case(B, kmax, total_q, seed, all_inactive=False):
    rng = np.random.default_rng(seed)
    seqlens = np.where(rng.random(B) < 0.2, -1, rng.integers(0, 50, B)).astype(np.int32)
    if all_inactive:
        seqlens[:] = -1
    draft_len = rng.integers(0, kmax + 1, B).astype(np.int32)
    drafts = rng.integers(0, 1000, (B, kmax)).astype(np.int32)
    for b in range(B):
        drafts[b, draft_len[b]:] = -1
    return rng.integers(0, 1000, B).astype(np.int32), drafts, draft_len, seqlens, total_q


@pytest.mark.parametrize("name,case", [
    ("total_q_is_B", _pack_case(6, 4, 6, 1)),
    ("budget_ends_inside_a_slot", _pack_case(6, 4, 6 + 5, 2)),
    ("budget_larger_than_needed", _pack_case(6, 4, 6 * 5 + 9, 3)),
    ("all_inactive", _pack_case(6, 4, 17, 4, all_inactive=True)),
    ("B_1", _pack_case(1, 4, 3, 5)),
    ("B_1025", _pack_case(1025, 3, 1025 + 700, 6)),
    ("kmax_0", _pack_case(5, 0, 8, 7)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_pack_against_the_oracle(name, case):
    last, drafts, draft_len, seqlens, total_q = case
    B = last.size
    if name == "budget_ends_inside_a_slot":
        seqlens[:] = 10
        draft_len[:] = [3, 4, 2, 0, 4, 1]          # 5 extra rows: 3 to slot 0, 2 of slot 1's 4, nothing behind
    w_cu, w_ids, w_drafts, w_len = S.pack(last, drafts, draft_len, seqlens, total_q)
    if name == "budget_ends_inside_a_slot":
        assert w_len.tolist() == [3, 2, 0, 0, 0, 0] and w_cu.tolist() == [0, 4, 7, 8, 9, 10, 11]
    if name == "budget_larger_than_needed":
        assert w_cu[-1] < total_q
    cu, check_cu = _guarded(B + 1)
    ids, check_ids = _guarded(total_q)
    d_drafts, d_len = _dev(drafts), _dev(draft_len)
    ops.spec_pack(_dev(last), d_drafts, d_len, _dev(seqlens), total_q, cu_seqlens_q=cu, input_ids=ids)
    assert np.array_equal(_np(cu), w_cu) and np.array_equal(_np(ids), w_ids)
    assert np.array_equal(_np(d_len), w_len) and np.array_equal(_np(d_drafts), w_drafts)
    check_cu(), check_ids()
    if name == "all_inactive":
        assert (_np(cu) == 0).all() and (_np(ids) == -1).all()


# ------------------------------------------------------------------------------------------------------------------------
# the verifier
# ------------------------------------------------------------------------------------------------------------------------
BURSTS = (1, 2, 5, 0)   # rows per slot, in rotation over the slots (one slot per sampler mode); three padding rows behind
_VERIFY = {}


def _verify_case(V, dtype_name):
    """One slot per mode of sample_oracle.MODES with the mode's parameters, history and (placed) p and u; slot i brings BURSTS[i % 4] rows, every
    one the mode's own logits row, so p and u keep their margins.  The inputs behind a slot's first row are ids the slot's history already holds
    (small V), or the row's least likely tokens (their penalty moves no threshold by 1e-4), and one id outside [0, V).  -> arrays + the oracle's
    row tokens, shared by the tests and never written."""
    key = (V, dtype_name)
    if key in _VERIFY:
        return _VERIFY[key]
    case = SO.build_case(V, dtype_name)
    M = len(SO.MODES)
    n = np.array([BURSTS[i % len(BURSTS)] for i in range(M)])
    cu = np.zeros(M + 1, np.int32)
    cu[1:] = np.cumsum(n)
    T = int(cu[-1]) + 3
    lf = case["logits"].float().numpy()
    src = np.zeros(T, np.int64)
    ids = np.full(T, -1, np.int32)
    u = np.zeros(T, np.float32)
    for i in range(M):
        hist = case["history"][i, :case["hist_len"][i]]
        inside = hist[(hist >= 0) & (hist < V)]
        rare = np.argsort(lf[i], kind="stable")[:4]
        for j in range(n[i]):
            r = cu[i] + j
            src[r], u[r] = i, case["u"][i]
            if j == 0:
                ids[r] = (3 * i + 1) % V
            elif j == 3:
                ids[r] = V + 2
            elif not case["r"][i] > 1:
                ids[r] = (7 * j + i) % V                 # no penalty: any id
            elif V >= 1000:
                ids[r] = rare[j - 1]                     # new ids, counted (hist_len + j - 1 < Lh) and harmless to the thresholds
            else:
                ids[r] = inside[j % inside.size] if inside.size else V + 2 + j
    logits = case["logits"][torch.from_numpy(src)].contiguous()
    logits[cu[-1]:] = float("nan")        # padding rows are not read
    want, margin = S.verify(logits.float().numpy(), u, cu, ids, M, case["t"], case["k"], case["p"], case["r"], case["history"], case["hist_len"])
    out = dict(case=case, cu=cu, ids=ids, u=u, logits=logits, want=want, margin=margin, T=T, M=M)
    _VERIFY[key] = out
    return out


def _run_verify(c, u=None, eng=None):
    case = c["case"]
    kw = dict(temperature=_dev(case["t"]), top_k=_dev(case["k"]), top_p=_dev(case["p"]), repetition_penalty=_dev(case["r"]),
              history=_dev(case["history"]), hist_len=_dev(case["hist_len"]))
    return _np((eng or ops).spec_verify(_dev(c["logits"]), _dev(c["u"] if u is None else u), _dev(c["cu"]), _dev(c["ids"]), **kw))


VERIFY_SHAPES = [(V, d) for V in (1, 7, 257, 4099) for d in ("fp32", "bf16", "fp16")] + [(128256, "bf16")]


@pytest.mark.parametrize("V,dtype_name", VERIFY_SHAPES)
def test_verify_equals_the_oracle_on_every_mode_and_burst(V, dtype_name):
    c = _verify_case(V, dtype_name)
    live = np.arange(c["T"]) < c["cu"][-1]
    assert (c["margin"][live] >= SO.MARGIN).all(), c["margin"]
    got = _run_verify(c)
    assert np.array_equal(got, c["want"]), (np.flatnonzero(got != c["want"]), got, c["want"])
    assert (got[~live] == -1).all() and ((got[live] >= 0) & (got[live] < V)).all()


def _verify_against_sample_logits(c, seed):
    """the same rows through ops.sample_logits, the owner's parameters replicated per row and the penalty set written out as the row's history:
    the same routine on the same bits, so ARBITRARY uniforms must give equal tokens"""
    case, cu, ids, T, M = c["case"], c["cu"], c["ids"], c["T"], c["M"]
    live = int(cu[-1])
    u = np.random.default_rng(seed).random(T).astype(np.float32)
    own = np.array([S.owner(cu, M, r) for r in range(live)])
    Lh = case["history"].shape[1]
    hist, hl = np.zeros((live, Lh + 8), np.int32), np.zeros(live, np.int32)
    for r in range(live):
        b = own[r]
        ps = S.penalty_set(case["history"][b], case["hist_len"][b], ids, int(cu[b]), r - int(cu[b]))
        hist[r, :len(ps)] = ps
        hl[r] = len(ps)
    want = _np(ops.sample_logits(_dev(c["logits"][:live]), _dev(u[:live]), temperature=_dev(case["t"][own]), top_k=_dev(case["k"][own]),
                                 top_p=_dev(case["p"][own]), repetition_penalty=_dev(case["r"][own]), history=_dev(hist), hist_len=_dev(hl)))
    got = _run_verify(c, u=u)
    assert np.array_equal(got[:live], want), np.flatnonzero(got[:live] != want)
    # and without a history or any parameter at all: t = 1, no filter, no penalty
    plain = _np(ops.spec_verify(_dev(c["logits"]), _dev(u), _dev(cu), _dev(ids)))
    assert np.array_equal(plain[:live], _np(ops.sample_logits(_dev(c["logits"][:live]), _dev(u[:live])))) and (plain[live:] == -1).all()


@pytest.mark.parametrize("V,dtype_name", VERIFY_SHAPES)
def test_verify_equals_sample_logits_with_no_margin(V, dtype_name):
    _verify_against_sample_logits(_verify_case(V, dtype_name), V)


@pytest.mark.parametrize("V,dtype_name", SO.EDGE_SHAPES)
def test_verify_equals_the_oracle_on_the_edge_rows(V, dtype_name):
    """sample_oracle's edge rows (flat heads, dense runs, the +-0 group: the rows that tests/test_sample_host.py proves sensitive to every fault
    of MUTANTS) as bursts of 1, 2 and 5 rows per slot under the slot's parameters and history: the oracle's tokens, which are the sampler's"""
    c = S.edge_verify_case(V, dtype_name)
    live = np.arange(c["T"]) < c["cu"][-1]
    assert (c["margin"][live] >= SO.MARGIN).all() and np.array_equal(c["want"][live], c["grid"][live])
    got = _run_verify(c)
    assert np.array_equal(got, c["want"]), (np.flatnonzero(got != c["want"]), got, c["want"])


@pytest.mark.parametrize("V,dtype_name", SO.EDGE_SHAPES)
def test_verify_equals_sample_logits_on_the_edge_rows(V, dtype_name):
    _verify_against_sample_logits(S.edge_verify_case(V, dtype_name), V)


@pytest.mark.parametrize("V,dtype_name", [(1025, "fp32"), (1025, "bf16")])
def test_a_burst_whose_earlier_inputs_are_the_whole_penalty_set(V, dtype_name):
    """32 slots of five rows on the two ladders, penalty 1.5, empty histories: the top head id, V + (a head id), the top id again and another head id
    enter the penalty set row by row.  tests/test_spec_host.py proves that a wrapped id and a penalty per occurrence change these tokens."""
    c = S.penalty_burst_case(V, dtype_name)
    assert (c["margin"] >= SO.MARGIN).all()
    got = _run_verify(c)
    assert np.array_equal(got, c["want"]), (np.flatnonzero(got != c["want"]), got, c["want"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_an_earlier_input_of_the_burst_is_penalised_unless_the_history_is_full(dtype):
    """greedy, penalty 2: token 5 (logit 4) beats token 9 (logit 3) until 5 is in the penalty set (4 / 2 < 3).  The slot's history does not hold 5;
    the burst's second input is 5.  Row 0 draws 5, row 1 must draw 9 -- but not when the history is full, for the serial loop could not have
    appended the 5 then."""
    V, Lh = 257, 8
    x = torch.zeros(4, V)
    x[:, 5], x[:, 9] = 4.0, 3.0
    cu = np.array([0, 2, 4], np.int32)
    ids = np.array([7, 5, 7, 5], np.int32)
    history = np.array([[1, 2, 3, 4, 6, 8, 10, 11]] * 2, np.int32)
    hist_len = np.array([2, Lh], np.int32)                  # slot 0: room for the 5; slot 1: full
    t, k, p, r = np.zeros(2, np.float32), np.zeros(2, np.int32), np.ones(2, np.float32), np.full(2, 2.0, np.float32)
    want, _ = S.verify(x.numpy(), np.full(4, 0.5, np.float32), cu, ids, 2, t, k, p, r, history, hist_len)
    assert want.tolist() == [5, 9, 5, 5]
    got = ops.spec_verify(_dev(x, dtype), _dev(np.full(4, 0.5, np.float32)), _dev(cu), _dev(ids), temperature=_dev(t), top_k=_dev(k), top_p=_dev(p),
                          repetition_penalty=_dev(r), history=_dev(history), hist_len=_dev(hist_len))
    assert _np(got).tolist() == [5, 9, 5, 5]
    hist_len[1] = Lh - 1                                    # the last free place: the 5 goes in, the row after it sees it
    got = ops.spec_verify(_dev(x, dtype), _dev(np.full(4, 0.5, np.float32)), _dev(cu), _dev(ids), temperature=_dev(t), top_k=_dev(k), top_p=_dev(p),
                          repetition_penalty=_dev(r), history=_dev(history), hist_len=_dev(hist_len))
    assert _np(got).tolist() == [5, 9, 5, 9]


# ------------------------------------------------------------------------------------------------------------------------
# the accept chain
# ------------------------------------------------------------------------------------------------------------------------
def _accept_case():
    """seven slots, kmax 4, Lh 8, max_len 30, stop id 99:
    0 every draft stands (the bonus token) | 1 the first draft falls | 2 a stop id among the standing drafts | 3 max_len inside the burst |
    4 the history fills inside the burst | 5 no rows | 6 one row (a plain decode)"""
    kmax = 4
    inputs = [[10, 11, 12, 13, 14], [20, 21, 22], [30, 31, 99, 33], [40, 41, 42, 43], [50, 51, 52, 53], [], [70]]
    sampled = [[11, 12, 13, 14, 15], [25, 22, 23], [31, 99, 33, 34], [41, 42, 43, 44], [51, 52, 53, 57], [], [71]]
    cu = np.zeros(8, np.int32)
    cu[1:] = np.cumsum([len(x) for x in inputs])
    T = int(cu[-1]) + 2
    ids, rt = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
    ids[:cu[-1]], rt[:cu[-1]] = np.concatenate(inputs), np.concatenate(sampled)
    state = dict(history=np.arange(56, dtype=np.int32).reshape(7, 8) + 200, hist_len=np.array([1, 2, 3, 0, 6, 4, 9], np.int32),
                 seqlens=np.array([5, 6, 7, 27, 9, 10, 11], np.int32), finished=np.zeros(7, np.int32))
    return kmax, cu, ids, rt, state


@pytest.mark.parametrize("append,advance", [(True, True), (False, True), (True, False), (False, False)])
def test_accept_against_the_oracle(append, advance):
    kmax, cu, ids, rt, state = _accept_case()
    want_state = {k: v.copy() for k, v in state.items()}
    w_out, w_num, w_last = S.accept(rt, ids, cu, kmax, want_state["history"], want_state["hist_len"], want_state["seqlens"], [99, 1000],
                                    want_state["finished"], 30, append, advance)
    if append and advance:   # the oracle's answers, by hand
        assert w_num.tolist() == [5, 1, 2, 3, 4, 0, 1] and w_last.tolist() == [15, 25, 99, 43, 57, -1, 71]
        assert want_state["seqlens"].tolist() == [10, 7, -1, -1, 13, 10, 12] and want_state["finished"].tolist() == [0, 0, 1, 0, 0, 0, 0]
        assert want_state["hist_len"].tolist() == [6, 3, 5, 3, 10, 4, 10] and want_state["history"][4, 6:].tolist() == [51, 52]
    dev = {k: _dev(v) for k, v in state.items()}
    out, check_out = _guarded(7, kmax + 1)
    num, check_num = _guarded(7)
    last, check_last = _guarded(7)
    ops.spec_accept(_dev(rt), _dev(ids), _dev(cu), kmax, stop_ids=_dev(np.array([99, 1000], np.int32)), max_len=30, append=append, advance=advance,
                    out_tokens=out, num_emitted=num, last_tokens=last, **dev)
    assert np.array_equal(_np(out), w_out) and np.array_equal(_np(num), w_num) and np.array_equal(_np(last), w_last), (_np(out), w_out)
    for k in state:
        assert np.array_equal(_np(dev[k]), want_state[k]), (k, _np(dev[k]), want_state[k])
    check_out(), check_num(), check_last()


# ------------------------------------------------------------------------------------------------------------------------
# the loop on the toy model: ops.sample_logits token by token against PromptLookupSampler
# ------------------------------------------------------------------------------------------------------------------------
class _Toy:
    """the toy model and both loops on the device; every tensor a step touches is persistent, so a step can be captured"""

    def __init__(self, s):
        self.s = s
        B, V = S.TOY_B, S.TOY_V
        self.table, self.u_tab = _dev(s["table"]), _dev(s["u_tab"])
        self.smp = DeviceSampler(B, V, DEV, max_history=S.TOY_LH, stop_ids=s["stop_ids"].tolist(), max_len=s["max_len"])
        self.smp.temperature.copy_(_dev(S.TOY_PARAMS["t"]))
        self.smp.top_k.copy_(_dev(S.TOY_PARAMS["k"]))
        self.smp.top_p.copy_(_dev(S.TOY_PARAMS["p"]))
        self.smp.repetition_penalty.copy_(_dev(S.TOY_PARAMS["r"]))
        self.seqlens = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.spec = PromptLookupSampler(self.smp, self.seqlens, kmax=S.TOY_KMAX, ngram_min=1, ngram_max=3)
        self.rows = torch.arange(self.spec.total_q, device=DEV)
        self.slots = torch.arange(B, device=DEV)
        self.reset()

    def reset(self):
        s = self.s
        self.smp.history.copy_(_dev(s["history"]))
        self.smp.hist_len.copy_(_dev(s["hist_len"]))
        self.smp.finished.zero_()
        self.seqlens.copy_(_dev(s["seqlens"]))
        self.spec.set_last_tokens(_dev(s["last_tokens"]))

    def state(self):
        return {k: _np(v).copy() for k, v in (("history", self.smp.history), ("hist_len", self.smp.hist_len), ("seqlens", self.seqlens),
                                               ("finished", self.smp.finished))}

    def serial(self, steps=S.TOY_STEPS):
        """-> (tokens [steps, B], steps until every slot has finished)"""
        last, toks, done = _dev(self.s["last_tokens"]), [], steps
        for it in range(steps):
            logits = self.table[last.clamp(min=0).long()]
            u = self.u_tab[self.slots, self.seqlens.clamp(min=0).long()]
            last = self.smp(logits, seqlens=self.seqlens, u=u)
            toks.append(_np(last))
            if done == steps and (self.seqlens < 0).all():
                done = it + 1
        return np.stack(toks), done

    def spec_step(self):
        """draft -> pack -> table gather -> verify -> accept, nothing read on the host"""
        ids, cu = self.spec.begin_step()
        B = S.TOY_B
        own = torch.bucketize(self.rows, cu[1:].long(), right=True).clamp(max=B - 1)       # the last b with cu[b] <= r (padding rows: any slot)
        pos = (self.seqlens[own].long() + self.rows - cu[own].long()).clamp(min=0, max=self.u_tab.shape[1] - 1)
        logits = self.table[ids.clamp(min=0).long()]
        return self.spec.end_step(logits, u=self.u_tab[own, pos])


def _spec_eager(toy, steps=S.TOY_STEPS):
    outs, nums, done = [], [], steps
    for it in range(steps):
        out, num = toy.spec_step()
        outs.append(_np(out).copy())
        nums.append(_np(num).copy())
        if done == steps and (toy.seqlens < 0).all():
            done = it + 1
    return np.stack(outs), np.stack(nums), done


@pytest.mark.parametrize("make", [S.toy_state, S.toy_state_with_stop], ids=["max_len", "stop_id"])
def test_speculative_loop_emits_what_the_serial_loop_emits_in_fewer_steps(make):
    """V = 257, B = 3 (greedy; temperature + top-k + top-p; repetition penalty), 40 steps, kmax 4, uniforms by absolute position"""
    toy = _Toy(make(0))
    toks, serial_steps = toy.serial()
    want = toy.state()
    toy.reset()
    outs, nums, spec_steps = _spec_eager(toy)
    got = toy.state()
    assert S.stream(outs) == S.stream(toks)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert (want["seqlens"] == -1).all() and spec_steps < serial_steps, (spec_steps, serial_steps)
    assert np.array_equal(nums, (outs >= 0).sum(-1)) and (nums.sum(0) > (nums > 0).sum(0)).all()
    if make is S.toy_state_with_stop:
        assert want["finished"].any()


def test_one_captured_step_replays_the_eager_loop():
    toy = _Toy(S.toy_state_with_stop(0))
    e_out, e_num, _ = _spec_eager(toy)
    want = toy.state()
    toy.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        toy.spec_step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    toy.reset()
    with torch.cuda.graph(graph):
        out, num = toy.spec_step()
    for _ in range(2):       # with the eager run: three runs, identical outputs
        toy.reset()
        outs, nums = [], []
        for it in range(S.TOY_STEPS):
            graph.replay()
            outs.append(_np(out).copy())
            nums.append(_np(num).copy())
        assert np.array_equal(np.stack(outs), e_out) and np.array_equal(np.stack(nums), e_num)
        got = toy.state()
        for k in want:
            assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# cache bookkeeping: rejected rows need no rollback
# ------------------------------------------------------------------------------------------------------------------------
HID, H, HKV, DH, L = 256, 4, 2, 64, 256
W = (H + 2 * HKV) * DH


def _module(kv_dtype):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused
    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=HKV, hidden_size=HID, rope_theta=10000.0, rope_scaling=None,
                           max_position_embeddings=L)
    # the projections are stand-ins: x already is the qkv tensor and the output is returned as it is
    return QuantLlamaAttentionFused(HID, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=2, kv_layout="natural",
                                    kv_dtype=kv_dtype)


@pytest.mark.parametrize("kv_dtype,dtype", [(None, torch.float16), ("fp8", torch.bfloat16)], ids=["T-f16", "fp8-bf16"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_the_step_after_a_partly_rejected_burst_reads_accepted_tokens_only(kv_dtype, dtype, paged):
    """slot 0 (70 tokens) brings 1 + 3 rows of which two are emitted, slot 1 (5 tokens) one row.  The next step on that cache must equal, bit for
    bit, the same call on a cache that was only ever given the accepted rows (zeros beyond the lengths)."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(L, device=DEV).float(), inv)
    freqs = torch.cat([f, f], -1).contiguous()
    g = torch.Generator(device=DEV).manual_seed(7)
    draw = lambda n: (torch.randn(1, n, W, generator=g, device=DEV)).to(dtype)
    kw = {}
    if paged:
        ps = 64
        kw = dict(block_table=torch.randperm(2 * L // ps, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(2, -1).to(DEV), page_size=ps)
    spec, clean = _module(kv_dtype), _module(kv_dtype)
    kmax, hist = 4, (70, 5)
    step = lambda m, x, pos, cu: m.forward_packed_split(x, _dev(np.array(pos, np.int32)), freqs, _dev(np.array(cu, np.int32)), kmax + 1,
                                                        split_seqlen_q=kmax + 1, split_min_keys=64, **kw)
    xh = draw(sum(hist))
    for m in (spec, clean):      # the histories, as one packed prompt step
        m.forward_packed(xh, _dev(np.array([0, 0], np.int32)), freqs, _dev(np.array([0, 70, 75], np.int32)), 70, **kw)
    x1 = draw(5 + 3)             # rows 0 .. 3: slot 0's burst; row 4: slot 1; three padding rows
    step(spec, x1, hist, [0, 4, 5])
    x1_acc = torch.cat([x1[:, 0:2], x1[:, 4:5], x1[:, 5:]], 1)     # what the accept step kept: slot 0's rows 0 and 1, slot 1's row
    step(clean, x1_acc, hist, [0, 2, 3])
    x2 = draw(3 + 2 + 2)
    pos2, cu2 = (72, 6), [0, 3, 5]
    got, want = step(spec, x2, pos2, cu2), step(clean, x2, pos2, cu2)
    torch.cuda.synchronize()
    assert torch.isfinite(want[0, :5].float()).all() and want[0, :5].float().abs().sum() > 0
    assert torch.equal(got[0, :5].contiguous().view(torch.int16), want[0, :5].contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------
# the torch-extension entries
# ------------------------------------------------------------------------------------------------------------------------
def test_engine_bindings_give_the_bits_of_ops():
    eng = llm_awq_amd.load_engine()
    history, hist_len, seqlens, max_draft, want, want_len = S.draft_case_arrays(list(range(8)))
    drafts, draft_len = eng.spec_draft_ngram(_dev(history), _dev(hist_len), _dev(seqlens), max_draft=_dev(max_draft), **S.DRAFT_KW)
    assert np.array_equal(_np(drafts), want) and np.array_equal(_np(draft_len), want_len)
    last = np.arange(8, dtype=np.int32) + 500
    w_cu, w_ids, w_drafts, w_len = S.pack(last, want, want_len, seqlens, 8 + 6)
    cu, ids = eng.spec_pack(_dev(last), drafts, draft_len, _dev(seqlens), 8 + 6)
    assert np.array_equal(_np(cu), w_cu) and np.array_equal(_np(ids), w_ids) and np.array_equal(_np(draft_len), w_len)
    c = _verify_case(257, "fp16")
    assert np.array_equal(_run_verify(c, eng=eng), c["want"])
    kmax, cu, ids, rt, state = _accept_case()
    a, b = {k: _dev(v) for k, v in state.items()}, {k: _dev(v) for k, v in state.items()}
    stop = _dev(np.array([99], np.int32))
    got = eng.spec_accept(_dev(rt), _dev(ids), _dev(cu), kmax, stop_ids=stop, max_len=30, append=True, advance=True, **a)
    ref = ops.spec_accept(_dev(rt), _dev(ids), _dev(cu), kmax, stop_ids=stop, max_len=30, append=True, advance=True, **b)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    for k in state:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(RuntimeError):
        eng.spec_verify(_dev(c["logits"]), _dev(c["u"][:3]), _dev(c["cu"]), _dev(c["ids"]))
