"""not-gpu: the device-sampling contract on the host -- the numpy oracle (tests/sample_oracle.py) against hand-worked rows and against the four HF
logits processors the reference's loop runs (tinychat/stream_generators/stream_gen.py:19-32), the robustness of every row the builders make, the proof that the edge rows of the
GPU tests tell every fault of sample_oracle.MUTANTS from the contract, and the C entry's argument checks, which need no launch."""
import ctypes

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi
from tests import sample_oracle as O


def test_oracle_on_hand_worked_rows():
    # masses 1, 1/2, 1/4, 1/4 of the top (logits in units of ln 2): probabilities 1/2, 1/4, 1/8, 1/8
    ln2 = np.log(2.0)
    x = np.array([-1.0, 0.0, -2.0, -2.0], dtype=np.float64) * ln2
    row = O.Row(O.process(x))
    assert row.argmax == 1
    np.testing.assert_allclose(row.S_above, [0.0, 0.5, 0.75], atol=1e-7)       # three tie groups: {1}, {0}, {2, 3}
    assert list(row.N_above) == [0, 1, 2]
    assert list(row.kept(0.6, 0)[0]) == [True, True, False, False]             # S = 0, 0.5 < 0.6 <= 0.75
    assert row.kept(0.6, 0)[1] == pytest.approx(0.1, abs=1e-6)                 # p is 0.1 from S = 0.5
    assert list(row.kept(0.8, 0)[0]) == [True, True, True, True]               # the tie group {2, 3} is kept whole
    assert list(row.kept(1.0, 3)[0]) == [True, True, True, True]               # top-k 3 reaches into the tie group: whole group
    assert list(row.kept(1.0, 2)[0]) == [True, True, False, False]
    assert list(row.kept(1.0, 1)[0]) == [False, True, False, False]
    assert list(row.kept(0.8, 1)[0]) == [False, True, False, False]            # the tighter filter cuts
    # all kept, index order: C = 1/4, 3/4, 7/8, 1 (of Zk); the first C_v > u
    mask = np.ones(4, bool)
    toks, margins = row.draw(mask, [0.0, 0.2, 0.25, 0.5, 0.8, 0.9, 0.999])
    assert list(toks) == [0, 0, 1, 1, 2, 3, 3]
    assert margins[1] == pytest.approx(0.05, abs=1e-6) and margins[3] == pytest.approx(0.25, abs=1e-6) and margins[2] == pytest.approx(0.0, abs=1e-7)
    # kept {0, 1}: C = 1/3, 1 of Zk
    toks, _ = row.draw(row.kept(0.6, 0)[0], [0.3, 0.34])
    assert list(toks) == [0, 1]
    # the whole contract through sample_row: greedy by either threshold, lowest index among the maxima
    assert O.sample_row(np.array([1.0, 3.0, 3.0, 2.0]), 0.9, t=0.0)[0] == 1
    assert O.sample_row(np.array([1.0, 3.0, 3.0, 2.0]), 0.9, t=0.5, p=0.0)[0] == 1
    assert O.sample_row(np.zeros(5), 0.9, t=0.0)[0] == 0


def test_oracle_temperature_and_penalty_are_float32():
    x = np.array([3.0, -1.5, 0.7, 2.0], dtype=np.float32)
    got = O.process(x, t=0.7, r=1.3, history=[0, 0, 1, 9, -2])
    t, r = np.float32(0.7), np.float32(1.3)
    want = np.array([(x[0] / t) / r, (x[1] / t) * r, x[2] / t, x[3] / t], dtype=np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert O.process(x, t=1.0).tobytes() == x.tobytes() and O.process(x, t=0.0).tobytes() == x.tobytes()   # no-op and greedy: no division
    assert O.process(x, t=0.7, r=1.0, history=[0]).tobytes() == (x / t).astype(np.float32).tobytes()
    assert O.advance(5, 10, 12, [7]) == (11, False) and O.advance(5, 10, 11, [7]) == (-1, False) and O.advance(7, 3, 100, [2, 7]) == (-1, True)


def test_oracle_keeps_what_the_hf_processors_keep_on_tie_free_rows():
    lp = pytest.importorskip("transformers.generation.logits_process")
    g = torch.Generator().manual_seed(5)
    V = 500
    for t, r, p, k in ((0.7, 1.0, 0.9, 0), (0.8, 1.3, 0.95, 40), (1.0, 1.2, 0.5, 100), (0.6, 1.0, 1.0, 7), (1.3, 1.1, 0.3, 3), (0.9, 1.0, 0.999, 0)):
        logits = torch.randn(1, V, generator=g) * 3.5            # fp32 draws: tie-free
        assert logits.unique().numel() == V
        hist = torch.randint(0, V, (1, 12), generator=g)
        procs = lp.LogitsProcessorList()                         # prepare_logits_processor's list and order
        if t >= 1e-5 and t != 1.0:
            procs.append(lp.TemperatureLogitsWarper(t))
        if r > 1.0:
            procs.append(lp.RepetitionPenaltyLogitsProcessor(r))
        if 1e-8 <= p < 1.0:
            procs.append(lp.TopPLogitsWarper(p))
        procs.append(lp.TopKLogitsWarper(k if k > 0 else V))
        hf = torch.isfinite(procs(hist, logits.clone())[0]).numpy()
        row = O.Row(O.process(logits[0].numpy(), t, r, hist[0].tolist()))
        mask, margin = row.kept(p, k)
        if margin < O.MARGIN:
            continue  # HF's fp32 cumulative sum may cut the other way that close to p
        assert np.array_equal(mask, hf), (t, r, p, k)


@pytest.mark.parametrize("V,dtype_name", [(V, d) for V, ds in O.SHAPES for d in ds])
def test_every_builder_row_is_robust(V, dtype_name):
    case = O.build_case(V, dtype_name)
    assert (case["margin"] >= O.MARGIN).all(), case["margin"]
    assert ((case["token"] >= 0) & (case["token"] < V)).all()
    # the stored token is the contract's, recomputed row by row from the raw logits
    if V <= 32000:
        lf = case["logits"].float().numpy()
        for i in range(len(O.MODES)):
            h = case["history"][i, :case["hist_len"][i]].tolist()
            tok, margin, _ = O.sample_row(lf[i], case["u"][i], case["t"][i], case["p"][i], int(case["k"][i]), case["r"][i], h)
            assert tok == case["token"][i] and margin >= O.MARGIN, O.MODES[i]


def test_grid_rows_outside_the_margin_are_at_most_one_per_boundary():
    _, u, tok, margin = O.build_grid()
    assert (margin < O.MARGIN).sum() <= 50
    kept = np.unique(tok)
    assert 1 <= kept.size <= 50 and (np.diff(tok[np.argsort(u)]) >= 0).all()   # index order: the token never falls as u rises


# ------------------------------------------------------------------------------------------------------------------------
# the edge rows of the GPU tests, and the proof that they see every fault of sample_oracle.MUTANTS
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,dtype_name", O.EDGE_SHAPES)
def test_every_edge_row_keeps_the_margin_and_the_oracle_reproduces_it(V, dtype_name):
    """conditions on the builder, not measurements: every row of every configuration has margin >= MARGIN (none is excluded), the grid's two ends
    are u = 0 and u = 1 - 2^-24 as they are, and the contract recomputed from the raw logits (a fresh Row, no mutant) gives the stored tokens"""
    cfgs = O.build_edge_case(V, dtype_name)
    assert len(cfgs) == (17 if V >= 1000 else 14)
    for c in cfgs:
        assert c["u"].size == O.U_GRID + 2 and c["margin"].min() >= O.MARGIN, (c["name"], c["margin"].min())
        assert ((c["u"] >= 0) & (c["u"] < 1)).all() and ((c["token"] >= 0) & (c["token"] < V)).all()
        n = c["hist_len"]
        tok, margin, mask = O.sample_rows(c["logits"].float().numpy(), c["u"], c["t"], c["p"], c["k"], c["r"], c["history"][:n])
        assert np.array_equal(tok, c["token"]) and margin.min() >= O.MARGIN, c["name"]
        if mask is not None:
            assert c["u"][-2] == 0.0 and c["u"][-1] == np.float32(1.0 - 2.0 ** -24)
            kept = np.flatnonzero(mask & (O.Row(O.process(c["x"], c["t"], c["r"], c["history"][:n])).m > 0))
            assert tok[-2] == kept[0] and tok[-1] == kept[-1]            # the ends draw the first and the last kept token
            assert np.unique(tok).size >= 4                                # a flat head: the grid lands on many tokens
    if V >= 1000:   # tau of the dense fp32 rows is decided by the last select pass: its low key byte is not 0, and keys share the 24 bits above
        for c in cfgs:
            if c["family"] == "dense" and dtype_name == "fp32":
                keys = O.key_of(c["x"])
                tau = keys[c["row"].kept(c["p"], c["k"])[0]].min()
                assert tau & 0xFF and ((keys >> 8) == (tau >> 8)).sum() >= 2 and ((keys >> 16) == (tau >> 16)).sum() >= 200, c["name"]


def test_the_largest_edge_shape_is_the_smallest_with_a_second_pass_iteration():
    """the arithmetic behind V = 40965 (csrc/awq_sample_row.hpp: 1024 threads x 4 chunks of 8 logits per iteration, 512-logit tiles, 64 lanes)"""
    V = max(v for v, _ in O.EDGE_SHAPES)
    nchunks = (V + 7) // 8
    assert V == 32768 + 8192 + 5 and 4096 + 1024 < nchunks < 4096 + 2 * 1024   # the second iteration's group: one chunk full, one partly, two empty
    assert (nchunks + 63) // 64 > 64                                       # a lane of the tile-sum scan owns two tiles
    assert all((b * V * es) % 16 for b in (1, 2, 3) for es in (2, 4))      # the rows behind the first start off a 16-byte boundary
    heads = O.head_indices(V)
    assert {0, 7, 8, 63, 64, 511, 512, 513, 32767, 32768, V - 3, V - 1} == set(heads)


def _kills(c, mutant):
    """the grid rows of a configuration on which a kernel with the fault would return another token for certain: margin on both sides"""
    tok, margin = O.edge_tokens(c, mutant)
    return (tok != c["token"]) & (margin >= O.MARGIN) & (c["margin"] >= O.MARGIN)


@pytest.mark.parametrize("mutant", list(O.MUTANTS))
def test_every_fault_is_seen_by_the_edge_rows(mutant, capsys):
    """for every (dtype, V) with a row family that can express the fault (sample_oracle.can_express), some configuration of the GPU case list
    changes its token on at least three grid rows; the counts are printed per configuration (pytest -s, or the failure report)"""
    lines, missed = [], []
    for V, dtype_name in O.EDGE_SHAPES:
        cfgs = [c for c in O.build_edge_case(V, dtype_name) if O.can_express(mutant, c["family"], dtype_name)]
        if not cfgs:
            lines.append(f"{mutant:24s} {dtype_name} V={V}: no row family of this shape can express it")
            continue
        n = {c["name"]: int(_kills(c, mutant).sum()) for c in cfgs}
        lines.append(f"{mutant:24s} {dtype_name} V={V}: {sum(n.values())} killing rows  " + " ".join(f"{k}={v}" for k, v in n.items() if v))
        if max(n.values()) < 3:
            missed.append((dtype_name, V))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not missed, (mutant, missed)
    assert any("killing" in ln for ln in lines if " fp32 " in ln)          # every fault is expressible at least in fp32


def test_the_rows_of_build_case_do_not_see_five_of_the_faults():
    """The gap the edge rows close, pinned as a statement about build_case's rows (peaked rows, u in the middle of the widest interval): over its
    273 rows up to V = 151936, none changes its token under k+1, k-1, tie_cut_at_k, pen_wrap or pen_always_div.  Whoever strengthens build_case
    will see this fail, and may then drop it."""
    blind = dict.fromkeys(("k+1", "k-1", "tie_cut_at_k", "pen_wrap", "pen_always_div"), 0)
    seen = dict.fromkeys(("pen_per_occurrence", "no_renorm"), 0)
    rows = 0
    for V, dtypes in O.SHAPES:
        for dtype_name in dtypes if V <= 151936 else ():
            case = O.build_case(V, dtype_name)
            lf = case["logits"].float().numpy()
            for i in range(len(O.MODES)):
                h, n = case["history"][i], case["hist_len"][i]
                row = O.Row(O.process(lf[i], case["t"][i], case["r"][i], h[:n]))
                rows += 1
                for counts in (blind, seen):
                    for m in counts:
                        tok = O.sample_row(lf[i], case["u"][i], case["t"][i], case["p"][i], int(case["k"][i]), case["r"][i], h[:n], row=row, mutant=m)[0]
                        counts[m] += int(tok != case["token"][i])
    assert rows == 273 and not any(blind.values()), blind
    assert seen == {"pen_per_occurrence": 6, "no_renorm": 39}, seen       # (the mutants themselves are alive on these rows)


def test_mutants_on_hand_worked_rows():
    ln2 = np.log(2.0)
    # a tie group that straddles k: masses 1, 1/2, 1/2, 1/2, 1/4; top-k 2 reaches into {1, 2, 3} and keeps it whole: C = 1, 1.5, 2, 2.5
    x = np.array([0.0, -1.0, -1.0, -1.0, -2.0]) * ln2
    row = O.Row(O.process(x))
    assert list(row.kept(1.0, 2)[0]) == [True, True, True, True, False]
    assert list(row.kept(1.0, 2, "tie_cut_at_k")[0]) == [True, True, False, False, False]
    assert list(row.kept(1.0, 2, "k-1")[0]) == [True, False, False, False, False]
    assert list(row.kept(1.0, 2, "k+1")[0]) == [True, True, True, True, False]          # k + 1 = 3 still ends inside the group
    assert list(row.kept(1.0, 4, "k+1")[0]) == [True] * 5 and list(row.kept(1.0, 4)[0]) == [True, True, True, True, False]
    assert O.sample_row(x, 0.7, k=2)[0] == 2 and O.sample_row(x, 0.7, k=2, mutant="tie_cut_at_k")[0] == 1      # 1.75 of 2.5; 1.05 of 1.5
    assert O.sample_row(x, 0.7, k=2, mutant="no_renorm")[0] == 2 and O.sample_row(x, 0.95, k=2, mutant="no_renorm")[0] == 3   # 0.95 * 2.75 > 2.5
    assert O.sample_row(x, 0.3, k=2, mutant="draw_sorted")[0] == 0 and O.sample_row(x, 0.3, k=2)[0] == 0
    # top-p 0.5 on probabilities 4/11, 2/11 x 3, 1/11: S = 0, 4/11, 10/11 -> the top two groups; one group more; the crossing group dropped
    assert list(row.kept(0.5, 0)[0]) == [True, True, True, True, False]
    assert list(row.kept(0.5, 0, "p_plus_group")[0]) == [True] * 5 and list(row.kept(0.5, 0, "p_drop_crossing")[0]) == [True, False, False, False, False]
    # the +-0 group: -0 and +0 are one value; the lowest index wins greedy; top-k 2 keeps all four zeros
    z = np.array([-0.0, -ln2, 0.0, -0.0, 0.0], dtype=np.float32)
    assert O.sample_row(z, 0.5, t=0.0)[0] == 0 and O.sample_row(z, 0.5, t=0.0, mutant="greedy_highest_index")[0] == 4
    zr = O.Row(O.process(z))
    assert list(zr.kept(1.0, 2)[0]) == [True, False, True, True, True]
    assert list(zr.kept(1.0, 2, "minus_zero_below")[0]) == [False, False, True, False, True]
    assert O.sample_row(z, 0.1, k=2)[0] == 0 and O.sample_row(z, 0.1, k=2, mutant="minus_zero_below")[0] == 2
    assert list(O.key_of(z)) == [0x80000000, O.key_of(np.float32(-ln2))[0], 0x80000000, 0x80000000, 0x80000000]
    # negative keys: -1 > -2 as values and as keys; by raw bits -2 ranks above -1
    n = np.array([-1.0, -2.0, -4.0], dtype=np.float32)
    assert list(np.argsort(O.key_of(n))) == [2, 1, 0] and list(np.argsort(O.key_of(n, flip_neg=False))) == [0, 1, 2]
    assert list(O.Row(n).kept(1.0, 1)[0]) == [True, False, False] and list(O.Row(n).kept(1.0, 1, "neg_raw_order")[0]) == [False, False, True]
    # a cleared low byte of tau takes in the keys that share tau's upper 24 bits
    d = np.array([0x3F800005, 0x3F800003, 0x3F800001, 0x3F7FFFFF], dtype=np.uint32).view(np.float32)
    assert list(O.Row(d).kept(1.0, 2)[0]) == [True, True, False, False]
    assert list(O.Row(d).kept(1.0, 2, "tau_low8")[0]) == [True, True, True, False] and list(O.Row(d).kept(1.0, 2, "tau_low16")[0]) == [True] * 3 + [False]
    # a negative logit under the penalty: multiplied; ids outside [0, V) ignored; once per distinct id
    x = np.array([-1.0, -2.0, 0.5], dtype=np.float32)
    hist = [0, 0, 2, 7, -1]
    assert O.process(x, r=2.0, history=hist).tolist() == [-2.0, -2.0, 0.25]
    assert O.process(x, r=2.0, history=hist, mutant="pen_always_div").tolist() == [-0.5, -2.0, 0.25]
    assert O.process(x, r=2.0, history=hist, mutant="pen_inverted").tolist() == [-0.5, -2.0, 1.0]
    assert O.process(x, r=2.0, history=hist, mutant="pen_per_occurrence").tolist() == [-4.0, -2.0, 0.25]
    assert O.process(x, r=2.0, history=hist, mutant="pen_wrap").tolist() == [-2.0, -4.0, 0.25]                # 7 -> 1; -1 -> 2, which is there already
    assert O.process(x, r=2.0, history=hist[:1], mutant="hist_len_ignored", stale=hist[1:]).tolist() == [-2.0, -2.0, 0.25]
    g = np.array([1.0, 0.9, -3.0], dtype=np.float32)
    assert O.sample_row(g, 0.5, t=0.0, r=2.0, history=[0])[0] == 1 and O.sample_row(g, 0.5, t=0.0, r=2.0, history=[0], mutant="greedy_ignores_penalty")[0] == 0


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    SHAPE, ALIGN, NULL, DTYPE = -4, -5, -6, -3
    names = ("logits", "u", "temperature", "top_k", "top_p", "penalty", "history", "hist_len", "seqlens", "stop_ids", "finished", "tokens")

    def call(B=2, V=100, dt=1, Lh=4, S=1, max_len=10, flags=3, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        return L.awq_sample_logits(a["logits"], dt, B, V, a["u"], a["temperature"], a["top_k"], a["top_p"], a["penalty"], a["history"], a["hist_len"],
                                   Lh, a["seqlens"], a["stop_ids"], S, a["finished"], max_len, flags, a["tokens"], None)

    for n in ("logits", "u", "tokens"):
        assert call(**{n: None}) == NULL, n
    assert call(history=None) == NULL and call(hist_len=None) == NULL          # a history comes with its lengths
    assert call(history=None, hist_len=None, flags=1) == NULL                  # append without a history
    assert call(seqlens=None, flags=2) == NULL                                 # advance without lengths
    assert call(stop_ids=None, S=1) == NULL
    assert call(dt=3) == DTYPE and call(dt=-1) == DTYPE
    assert call(B=0) == SHAPE and call(V=0) == SHAPE and call(V=(1 << 20) + 1) == SHAPE
    assert call(Lh=0) == SHAPE and call(S=-1) == SHAPE and call(flags=4) == SHAPE
    assert call(logits=p + 1) == ALIGN and call(dt=0, logits=p + 3) == ALIGN and call(dt=2, logits=p + 2) == ALIGN
    for n in names[1:]:
        assert call(**{n: p + 2}) == ALIGN, n


def test_ops_and_sampler_refuse_cpu_tensors_and_bad_shapes():
    from llm_awq_amd import ops
    logits, u = torch.zeros(2, 16), torch.zeros(2)
    with pytest.raises(_capi.AwqNativeError):
        ops.sample_logits(logits, u)
    import inspect
    assert list(inspect.signature(ops.sample_logits).parameters) == [
        "logits", "u", "temperature", "top_k", "top_p", "repetition_penalty", "history", "hist_len", "seqlens", "stop_ids", "finished", "max_len",
        "append", "advance"]
    import llm_awq_amd
    doc = llm_awq_amd.load_engine().sample_logits.__doc__.splitlines()[0]
    assert [s.split(":")[0].strip() for s in doc[doc.index("(") + 1:doc.rindex(")")].split(", ") if s.strip() != "*"] == list(
        inspect.signature(ops.sample_logits).parameters)
