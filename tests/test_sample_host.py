"""not-gpu: the device-sampling contract on the host -- the numpy oracle (tests/sample_oracle.py) against hand-worked rows and against the four HF
logits processors the reference's loop runs (tinychat/stream_generators/stream_gen.py:19-32), the robustness of every row the builders make, and the
C entry's argument checks, which need no launch."""
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
