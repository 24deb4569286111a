"""gpu: next-token sampling on the device (awq_sample_logits, ops.sample_logits, DeviceSampler) against the numpy oracle of the contract
(tests/sample_oracle.py), and its own replay inside a hipGraph.

Every row the builders make keeps its thresholds at least 1e-4 (of the row's mass) away from what they are compared with -- the margin derived in the
oracle's docstring from the fp32 exponent and the fixed-point masses -- so the token must EQUAL the oracle's, with no tolerance and no exclusions.
The grid test is the only one that leaves rows out (those within the margin of a boundary), and first bounds how many."""
import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from llm_awq_amd.sampling import DeviceSampler
from tests import sample_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _run_case(case, rows, **extra):
    """one launch over the given rows of a built case, every parameter its own tensor -> tokens (numpy)"""
    sel = torch.as_tensor(rows)
    kw = dict(temperature=_dev(case["t"][rows]), top_k=_dev(case["k"][rows]), top_p=_dev(case["p"][rows]), repetition_penalty=_dev(case["r"][rows]),
              history=_dev(case["history"][rows]), hist_len=_dev(case["hist_len"][rows]))
    kw.update(extra)
    return ops.sample_logits(_dev(case["logits"][sel]), _dev(case["u"][rows]), **kw).cpu().numpy()


@pytest.mark.parametrize("V,dtype_name", [(V, d) for V, ds in O.SHAPES for d in ds])
def test_every_mode_equals_the_oracle(V, dtype_name):
    """greedy by t and by p, temperature only, top-k 1 / 50 / V, top-p 0.5 / 0.95, both filters with either one binding, penalty 1.3 over a history
    with repeats and ids outside [0, V) and over an empty one: launched row by row, in threes and in eights (every launch a mixed batch)"""
    case = O.build_case(V, dtype_name)
    M = len(O.MODES)
    assert (case["margin"] >= O.MARGIN).all()
    for B in (1, 3, 8):
        for r0 in range(0, M, B):
            rows = np.arange(r0, min(r0 + B, M))
            got = _run_case(case, rows)
            want = case["token"][rows]
            assert np.array_equal(got, want), (B, [O.MODES[i] for i in rows[got != want]], got, want)


def test_null_parameters_switch_their_step_off():
    case = O.build_case(1025, "bf16")
    logits = _dev(case["logits"])
    i = O.MODES.index("plain")
    tok = ops.sample_logits(logits[i:i + 1], _dev(case["u"][i:i + 1])).cpu().numpy()   # nothing but logits and u: t = 1, no filter, no penalty
    assert tok[0] == case["token"][i]
    i = O.MODES.index("topk50")
    tok = ops.sample_logits(logits[i:i + 1], _dev(case["u"][i:i + 1]), temperature=_dev(case["t"][i:i + 1]), top_k=_dev(case["k"][i:i + 1])).cpu().numpy()
    assert tok[0] == case["token"][i]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_greedy_ties_go_to_the_lowest_index(dtype):
    V = 1025
    x = torch.full((4, V), 1.5, dtype=dtype)          # row 0: constant -> index 0
    x[1] = torch.randn(V).to(dtype)
    x[1, [900, 37, 512]] = 9.0                        # row 1: the maximum three times -> 37
    x[2] = -x[1]
    x[2, [1024, 1023]] = 10.0                         # row 2: in the scalar tail of the row
    x[3] = 0.0
    x[3, ::2] = -0.0                                  # row 3: -0 and +0 are one value -> index 0
    t0 = torch.zeros(4)
    for kw in (dict(temperature=_dev(t0)), dict(top_p=_dev(t0)), dict(temperature=_dev(t0), top_p=_dev(t0 + 0.9), top_k=_dev(torch.full((4,), 5, dtype=torch.int32)))):
        got = ops.sample_logits(_dev(x), _dev(torch.full((4,), 0.77)), **kw).cpu().tolist()
        assert got == [0, 37, 1023, 0], got


def test_u_grid_follows_the_distribution():
    """one row of V = 1000 under top-k 50, 2048 times with u = (i + 0.5) / 2048: every row outside the margin of a boundary equals the oracle, and at
    most one row per kept token is inside it -- so the histogram of the launch is the distribution's"""
    logits, u, want, margin = O.build_grid()
    N = u.size
    out = margin < O.MARGIN
    assert out.sum() <= 50
    got = ops.sample_logits(_dev(logits.expand(N, -1)), _dev(u), top_k=_dev(torch.full((N,), 50, dtype=torch.int32))).cpu().numpy()
    assert np.array_equal(got[~out], want[~out]), np.flatnonzero((got != want) & ~out)
    near = np.flatnonzero(out)   # inside the margin the neighbour across the boundary is the only other answer
    order = np.sort(np.unique(want))
    for i in near:
        j = np.searchsorted(order, want[i])
        assert got[i] in order[max(j - 1, 0):j + 2], i


def _launch_edge(picks, u=None):
    """one launch over the given grid rows of the given edge configurations, every parameter its own tensor; each row is its own copy of the
    configuration's logits, so for an odd V the rows behind the first start off a 16-byte boundary -> (tokens, the oracle's)"""
    rep = lambda name, dt: np.concatenate([np.repeat(np.asarray(c[name], dtype=dt)[None], len(i), 0) for c, i in picks])
    logits = torch.cat([c["logits"].expand(len(i), -1) for c, i in picks])
    got = ops.sample_logits(_dev(logits), _dev(np.concatenate([c["u"][i] for c, i in picks]) if u is None else u), temperature=_dev(rep("t", np.float32)),
                            top_k=_dev(rep("k", np.int32)), top_p=_dev(rep("p", np.float32)), repetition_penalty=_dev(rep("r", np.float32)),
                            history=_dev(rep("history", np.int32)), hist_len=_dev(rep("hist_len", np.int32))).cpu().numpy()
    return got, np.concatenate([c["token"][i] for c, i in picks])


def _mixed(cfgs):
    return [(c, (7 * ci + 11 * np.arange(5)) % (O.U_GRID + 2)) for ci, c in enumerate(cfgs)]


@pytest.mark.parametrize("V,dtype_name", O.EDGE_SHAPES)
def test_edge_rows_equal_the_oracle(V, dtype_name):
    """The rows whose kept set decides the token (sample_oracle.build_edge_case): ladders of twelve near-equal head tokens at the row's structural
    places, from 2.0 and from -1.0, under top-k 8 over a tie group / top-k 5 / top-p / penalty over a history with repeats, wrapping and stale
    ids / all of them / greedy; dense runs of consecutive values around 1, -1 and +-0 under a top-k whose tau the last select pass decides; a
    +-0 top group.  Each configuration is one launch of its 64-point u grid and u = 0, u = 1 - 2^-24; then five rows of every configuration in
    one mixed launch.  Token equality, no exclusions; tests/test_sample_host.py proves that each fault of MUTANTS changes some of these tokens."""
    cfgs = O.build_edge_case(V, dtype_name)
    every = np.arange(O.U_GRID + 2)
    for c in cfgs:
        assert c["margin"].min() >= O.MARGIN
        got, want = _launch_edge([(c, every)])
        assert np.array_equal(got, want), (c["name"], np.flatnonzero(got != want), got, want)
    got, want = _launch_edge(_mixed(cfgs))
    assert np.array_equal(got, want), (np.flatnonzero(got != want), got, want)


def test_the_edge_rows_of_the_two_iteration_shape_three_times():
    cfgs = O.build_edge_case(40965, "fp32")
    picks = _mixed(cfgs)
    u = torch.rand(5 * len(cfgs), generator=torch.Generator().manual_seed(5)).numpy()   # arbitrary u (no margin asked)
    (a, _), (b, _), (c, _) = (_launch_edge(picks, u=u) for _ in range(3))
    assert np.array_equal(a, b) and np.array_equal(a, c) and ((a >= 0) & (a < 40965)).all()
    (a, want), (b, _), (c, _) = (_launch_edge(picks) for _ in range(3))                   # and on the grid: the oracle's, three times
    assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want)


def test_inactive_rows_are_skipped_and_untouched():
    case = O.build_case(1023, "bf16")
    rows = np.arange(8)
    seq = np.array([5, -1, 7, -1, -1, 0, 3, -1], dtype=np.int32)
    hist, hl, sl, fin = _dev(case["history"][rows]), _dev(case["hist_len"][rows]), _dev(seq), _dev(np.zeros(8, np.int32))
    hist0, hl0 = hist.clone(), hl.clone()
    got = _run_case(case, rows, history=hist, hist_len=hl, seqlens=sl, finished=fin, stop_ids=_dev(np.array([-5], np.int32)), max_len=100, append=True,
                    advance=True)
    act = seq >= 0
    assert (got[~act] == -1).all() and np.array_equal(got[act], case["token"][rows][act])
    assert torch.equal(hist[~act], hist0[~act]) and torch.equal(hl[~act], hl0[~act]) and (sl.cpu().numpy()[~act] == -1).all()
    assert np.array_equal(sl.cpu().numpy()[act], seq[act] + 1) and np.array_equal(hl.cpu().numpy()[act], hl0.cpu().numpy()[act] + 1)
    assert fin.sum().item() == 0


def test_append_stop_advance_and_the_max_len_edge():
    case = O.build_case(1000, "fp32")
    rows = np.array([O.MODES.index(m) for m in ("topk50", "topp50", "temperature", "penalty", "greedy_t", "plain")])
    want = case["token"][rows]
    Lh = O.HIST_LEN
    hl_np = case["hist_len"][rows].copy()
    hl_np[1] = Lh           # a full history: nothing is stored, the length still counts on
    hl_np[2] = Lh - 1       # the last free place
    hist_np = case["history"][rows].copy()
    seq = np.array([3, 8, 9, 4, 8, 0], dtype=np.int32)
    stop = np.array([int(want[3]), int(want[0]), 10 ** 6], dtype=np.int32)   # rows 0 and 3 draw a stop id
    hist, hl, sl, fin = _dev(hist_np), _dev(hl_np), _dev(seq), _dev(np.zeros(6, np.int32))
    got = _run_case(case, rows, history=hist, hist_len=hl, seqlens=sl, finished=fin, stop_ids=_dev(stop), max_len=10, append=True, advance=True)
    # (the penalty row reads hist_len entries: rows 1 and 2 have penalty 1, so their longer histories change nothing)
    assert np.array_equal(got, want)
    new = [O.advance(int(t), int(s), 10, stop.tolist()) for t, s in zip(want, seq)]
    assert sl.cpu().tolist() == [n[0] for n in new] == [-1, 9, -1, -1, 9, 1]     # stop, 8 + 1 < 10, 9 + 1 >= 10, stop, 9, 1
    assert fin.cpu().tolist() == [int(n[1]) for n in new] == [1, 0, 0, 1, 0, 0]
    assert hl.cpu().tolist() == (hl_np + 1).tolist()
    h = hist.cpu().numpy()
    for i in range(6):
        exp = hist_np[i].copy()
        if hl_np[i] < Lh:
            exp[hl_np[i]] = want[i]
        assert np.array_equal(h[i], exp), i
    # without the flags nothing moves
    hist, hl, sl = _dev(hist_np), _dev(hl_np), _dev(seq)
    got = _run_case(case, rows, history=hist, hist_len=hl, seqlens=sl)
    assert np.array_equal(got, want) and hist.cpu().numpy().tolist() == hist_np.tolist() and hl.cpu().tolist() == hl_np.tolist() and sl.cpu().tolist() == seq.tolist()


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_bad_rows_stay_in_range_and_leave_the_others_exact(dtype_name):
    V = 1025
    case = O.build_case(V, dtype_name)
    rows = np.array([O.MODES.index(m) for m in ("topp95", "topk50", "temperature", "both_k_binds", "penalty", "topp50", "plain", "both_p_binds")])
    logits = case["logits"][torch.as_tensor(rows)].clone()
    bad = [1, 3, 4, 6]
    logits[1, 17] = float("nan")
    logits[3, 1000] = float("inf")
    logits[4] = float("-inf")
    logits[6, :] = float("nan")
    good = [i for i in range(8) if i not in bad]
    case2 = dict(case)
    for _ in range(2):
        got = ops.sample_logits(_dev(logits), _dev(case["u"][rows]), temperature=_dev(case["t"][rows]), top_k=_dev(case["k"][rows]),
                                top_p=_dev(case["p"][rows]), repetition_penalty=_dev(case["r"][rows]), history=_dev(case["history"][rows]),
                                hist_len=_dev(case["hist_len"][rows])).cpu().numpy()
        assert ((got >= 0) & (got < V)).all(), got
        assert np.array_equal(got[good], case2["token"][rows][good])
    # -inf logits have no mass: a row that is -inf but for three tokens draws among the three
    x = torch.full((1, V), float("-inf"))
    x[0, [5, 600, 1024]] = torch.tensor([0.0, 0.0, 0.0])
    for u, want in ((0.1, 5), (0.5, 600), (0.9, 1024)):
        assert ops.sample_logits(_dev(x.to(O.TORCH_DTYPES[dtype_name])), _dev(torch.tensor([u]))).item() == want


def test_the_same_call_three_times_gives_the_same_tokens():
    case = O.build_case(128256, "bf16")
    rows = np.arange(len(O.MODES))
    g = torch.Generator().manual_seed(3)
    u = torch.rand(len(rows), generator=g).numpy()   # arbitrary u (no margin asked): equal tokens from run to run all the same
    case = dict(case, u=u)
    a, b, c = (_run_case(case, rows) for _ in range(3))
    assert np.array_equal(a, b) and np.array_equal(a, c) and ((a >= 0) & (a < 128256)).all()


def test_eight_captured_steps_replay_the_eager_run():
    """eight sampling steps with append and advance, their u on the device, captured once and replayed twice from the same state = the eager run"""
    B, V, steps, Lh = 4, 32000, 8, 12
    g = torch.Generator().manual_seed(11)
    logits = _dev((torch.randn(steps, B, V, generator=g) * 3.5).to(torch.bfloat16))
    u = _dev(torch.rand(steps, B, generator=g))
    par = dict(temperature=_dev(torch.tensor([0.7, 1.0, 0.0, 0.9])), top_k=_dev(torch.tensor([50, 0, 10, 5], dtype=torch.int32)),
               top_p=_dev(torch.tensor([0.9, 1.0, 0.8, 0.95])), repetition_penalty=_dev(torch.tensor([1.3, 1.0, 1.2, 1.1])))
    init = dict(history=torch.zeros(B, Lh, dtype=torch.int32), hist_len=torch.tensor([0, 3, 5, 2], dtype=torch.int32),
                seqlens=torch.tensor([10, 20, -1, 13], dtype=torch.int32), finished=torch.zeros(B, dtype=torch.int32))
    init["history"][:, :5] = torch.randint(0, V, (B, 5), generator=g, dtype=torch.int32)
    state = {k: _dev(v.clone()) for k, v in init.items()}
    stop = _dev(torch.tensor([V + 1], dtype=torch.int32))

    def reset():
        for k, v in init.items():
            state[k].copy_(v)

    def run():
        return torch.stack([ops.sample_logits(logits[s], u[s], **par, **state, stop_ids=stop, max_len=16, append=True, advance=True) for s in range(steps)])

    reset()
    eager = run().cpu()
    want_state = {k: v.cpu().clone() for k, v in state.items()}
    assert (eager[:, 2] == -1).all() and want_state["seqlens"].tolist() == [-1, -1, -1, -1]   # rows 0, 1, 3 run into max_len = 16 on the way
    assert (eager[:6, 0] >= 0).all() and (eager[6:, 0] == -1).all()                            # 10 -> 15, then 15 + 1 >= 16: finished
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        reset()
        run()
    torch.cuda.current_stream().wait_stream(s)
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        toks = run()
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(toks.cpu(), eager)
        for k, v in state.items():
            assert torch.equal(v.cpu(), want_state[k]), k


def test_engine_binding_is_the_same_entry():
    case = O.build_case(1000, "fp16")
    rows = np.arange(len(O.MODES))
    eng = llm_awq_amd.load_engine()
    got = eng.sample_logits(_dev(case["logits"]), _dev(case["u"]), temperature=_dev(case["t"]), top_k=_dev(case["k"]), top_p=_dev(case["p"]),
                            repetition_penalty=_dev(case["r"]), history=_dev(case["history"]), hist_len=_dev(case["hist_len"])).cpu().numpy()
    assert np.array_equal(got, case["token"][rows])
    with pytest.raises(RuntimeError):
        eng.sample_logits(_dev(case["logits"]), _dev(case["u"][:3]))


def test_device_sampler_end_to_end():
    """three slots with their own parameters and prompts, four steps: every token, history and length equals the oracle run step by step"""
    V, B, steps = 1023, 3, 4
    lt, lf = O.make_logits(21, steps * B, V, "bf16")
    lt, lf = lt.view(steps, B, V), lf.reshape(steps, B, V)
    slots = [dict(temperature=0.7, top_p=0.9, top_k=40, repetition_penalty=1.3, prompt_ids=[int(np.argmax(lf[0, 0])), 5, 5, 900]),
             dict(temperature=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2, prompt_ids=[int(np.argmax(lf[0, 1]))]),
             dict(temperature=1.0, top_p=1.0, top_k=-1, repetition_penalty=1.0, prompt_ids=[])]
    smp = DeviceSampler(B, V, DEV, max_history=16, seed=1234)
    smp2 = DeviceSampler(B, V, DEV, max_history=16, seed=1234)
    for b, sl in enumerate(slots):
        smp.set_row(b, **sl)
        smp2.set_row(b, **sl)
    assert smp.top_k.cpu().tolist() == [40, V, V]
    hist = [list(sl["prompt_ids"]) for sl in slots]
    seqlens = _dev(torch.tensor([4, 1, 0], dtype=torch.int32))
    for s in range(steps):
        # u: placed by the oracle for the rows that draw (so the step is robust), and the sampler's own generator must be reproducible
        u = np.full(B, 0.5, np.float32)
        for b in (0, 2):
            sl = slots[b]
            row = O.Row(O.process(lf[s, b], sl["temperature"], sl["repetition_penalty"], hist[b]))
            p = O.place_p(row, 0.9) if b == 0 else 1.0
            if b == 0:
                smp.top_p[b] = p
                slots[b]["top_p"] = p
            u[b] = O.place_u(row, row.kept(p, max(sl["top_k"], 0))[0], 0.3 + 0.1 * s)
        got = smp(_dev(lt[s]).unsqueeze(1), seqlens=seqlens, u=_dev(u)).cpu().tolist()
        for b, sl in enumerate(slots):
            tok, margin, _ = O.sample_row(lf[s, b], u[b], sl["temperature"], sl["top_p"], max(sl["top_k"], 0), sl["repetition_penalty"], hist[b])
            assert margin >= O.MARGIN and got[b] == tok, (s, b)
            hist[b].append(tok)
        assert smp.hist_len.cpu().tolist() == [len(h) for h in hist]
        for b in range(B):
            assert smp.history[b, :len(hist[b])].cpu().tolist() == hist[b]
    assert seqlens.cpu().tolist() == [8, 5, 4]
    # its own u: the same seed draws the same tokens, all in range
    a = smp(_dev(lt[0])).cpu()
    smp2.history.copy_(smp.history)
    smp2.hist_len.copy_(smp.hist_len - 1)
    smp2.top_p.copy_(smp.top_p)
    c = smp2(_dev(lt[0])).cpu()
    assert torch.equal(a, c) and ((a >= 0) & (a < V)).all()


def test_from_gen_params_runs_the_single_sequence_loop():
    """the reference's gen_params -> a one-slot sampler: the prompt starts the history, every step appends, a stop id raises `finished`"""
    from types import SimpleNamespace
    V = 1000
    lt, lf = O.make_logits(33, 3, V, "fp16")
    prompt = [int(np.argmax(lf[0])), 3, 3]
    gp = SimpleNamespace(n_vocab=V, temp=0.0, top_p=0.95, top_k=40, repeat_penalty=1.3, n_predict=8)
    want = [O.sample_row(lf[0], 0.5, gp.temp, gp.top_p, gp.top_k, gp.repeat_penalty, prompt)[0]]
    want.append(O.sample_row(lf[1], 0.5, gp.temp, gp.top_p, gp.top_k, gp.repeat_penalty, prompt + want)[0])
    assert want[0] != prompt[0]                                    # (the penalty moved the greedy choice off the prompt's token)
    smp = DeviceSampler.from_gen_params(gp, DEV, prompt_ids=prompt, stop_ids=[want[1]])
    assert smp.history.shape == (1, len(prompt) + gp.n_predict) and smp.top_k.item() == 40 and smp.repetition_penalty.item() == pytest.approx(1.3)
    got = [smp(_dev(lt[s:s + 1]).view(1, 1, V)).item() for s in range(2)]
    assert got == want
    assert smp.history[0, :smp.hist_len.item()].cpu().tolist() == prompt + want and smp.finished.item() == 1
