"""not-gpu: the token log-probability contract on the host -- the numpy oracle (tests/lm_logprobs_oracle.py) against hand-worked rows, the invariants
of the plan and of the case list the GPU tests run, the proof that this list separates every oracle mutant from the contract by more than the derived
bound, the argument checks of the C entries (no launch needed) and evaluate.perplexity's window arithmetic against entry.py's loop restated in
torch float64."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from llm_awq_amd import _capi, evaluate, ops
from tests import lm_head_oracle as H
from tests import lm_logprobs_oracle as O


def _tiles():
    p = ops.lm_head_logprobs_plan(1, 1, 8)
    return p["row_tile"], p["vocab_tile"]


def test_oracle_on_hand_worked_rows():
    z = np.array([[0.0, 0.0, -np.inf, 0.0], [1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 1.0, 1.0]])
    r = O.from_logits(z, targets=[3, -1, 0], init={"lse": [9.0, 9.0, 9.0], "argmax": [7, 7, 7]})
    assert r["lse"][0] == math.log(3.0) and r["argmax"].tolist() == [0, 7, 0] and r["lse"][1] == 9.0           # row 1 is ignored: what it held
    assert r["target_logit"].tolist() == [0.0, 0.0, 5.0] and r["logprob"][0] == -math.log(3.0)
    assert abs(r["lse"][2] - (5.0 + math.log1p(3 * math.exp(-4.0)))) < 1e-15
    assert O.from_logits(z)["argmax"].tolist() == [0, 1, 0]                                                   # the LOWEST index among the maxima
    assert O.from_logits(z, mutant="argmax_highest_tie")["argmax"].tolist() == [3, 2, 0]
    for tg in (-1, -100, 4):
        assert not O.from_logits(z, targets=[0, tg, 0])["active"][1]
    # the whole contract from storage: two rows with ldx = 16, K = 8
    store = np.zeros(32)
    store[0:8] = [1, 2, 3, 4, 0, 0, 0, 0.5]
    store[16:24] = [-1, 0, 0, 0, 0, 0, 0, 2]
    w = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 4], [2, 0, 0, -1, 0, 0, 0, 0]], dtype=np.float64)
    bias = np.array([0.5, -1.0, 0.0])
    r = O.reference(store, 16, 2, w, bias, targets=[1, 1])
    assert r["z"].tolist() == [[10.5, 1.0, -2.0], [-0.5, 7.0, -2.0]] and r["target_logit"].tolist() == [1.0, 7.0] and r["argmax"].tolist() == [0, 1]
    assert abs(r["lse"][0] - math.log(math.exp(10.5) + math.exp(1.0) + math.exp(-2.0))) < 1e-14
    # round_logits: 257 -> 256 in bf16 before the log-sum-exp
    r = O.reference(np.array([257.0, 0, 0, 0, 0, 0, 0, 0]), 8, 1, np.eye(8)[:2], None, targets=[0], round_logits=True)
    assert r["target_logit"][0] == 256.0 and O.reference(np.array([257.0, 0, 0, 0, 0, 0, 0, 0]), 8, 1, np.eye(8)[:2], None, targets=[0],
                                                         round_logits=True, mutant="round_skipped")["target_logit"][0] == 257.0


def test_the_bound_is_the_derived_one():
    # one column: S = 1, log S = 0: the terms are the exponential's levels, the floor of the logarithm's ulp and the rounding of M + log S
    z = np.array([[3.0]])
    b = O.bounds(z, targets=[0], levels=4, n_tiles=1)
    want = 1.01 * (4 * (2.0 ** -23 + O.U) + 2.0 ** -126 + (1 + 1 - 1) * O.U) + math.log(2.0) * 2.0 ** -23 + O.U * 3.0
    assert b["lse"][0] == pytest.approx(want, rel=1e-12) and b["target_logit"][0] == 0.0
    assert b["logprob"][0] == pytest.approx(want + O.U * want, rel=1e-12)                  # z - lse = 0 here
    # the logit bound enters through its maximum over the row, the target's own through its element
    b2 = O.bounds(np.array([[3.0, 1.0]]), targets=[1], logit_bound=np.array([[0.25, 0.125]]))
    assert b2["lse"][0] > 0.25 and b2["target_logit"][0] == 0.125 and b2["logprob"][0] > 0.375
    # V equal logits: the argument of every exponential is 0, and the sum of V + tiles terms dominates
    V = 1 << 16
    b3 = O.bounds(np.zeros((1, V)), n_tiles=512, levels=4)["lse"][0]
    assert (V + 511) * O.U < b3 < 1.2 * (V + 512) * O.U + 4e-6 + 16 * 2.0 ** -23


def test_case_list_and_plan_invariants():
    rt, vt = _tiles()
    shapes = O.lattice_shapes(rt, vt)
    assert len(shapes) == 20
    assert {t for t, _, _ in shapes} == {1, 2, rt - 1, rt, rt + 1, 2 * rt + 5} and {v for _, v, _ in shapes} == {1, 17, vt - 1, vt, vt + 1, 2 * vt + 17}
    for k in O.K_VALUES:
        assert sum(1 for s in shapes if s[2] == k) >= 2
    assert max(k for _, _, k in shapes) * H.R * H.R + H.R < 2 ** 24
    for (t, v, k) in shapes + [(130, 2000, 4096), (300, 513, 8192), (3, 128256, 4096), (2047, 128256, 4096), (2047, 32000, 4096)]:
        p = ops.lm_head_logprobs_plan(t, v, k)
        assert (p["row_tile"], p["vocab_tile"]) == (rt, vt) and p["k_step"] == 64           # the tiles depend on nothing but the build
        assert p["blocks"] == -(-t // rt) * -(-v // vt)
        ws = ops.lm_head_logprobs_workspace_bytes(t, v, k)
        assert 3 * p["blocks"] * rt * 4 <= ws <= 3 * p["blocks"] * rt * 4 + 4 * (-(-t // rt)) * rt + 4 * 256
        assert ops.lm_head_logprobs_workspace_bytes(t, v, k, True) - ws == -(-(t * k * 2) // 256) * 256
    # the perplexity window against Llama-3's vocabulary: tens of megabytes, where the logits and their fp32 copy are 1.6 GB
    assert ops.lm_head_logprobs_workspace_bytes(2047, 128256, 4096) < 32 * 2 ** 20 < 2047 * 128256 * 6 // 32
    for bad in ((0, 10, 8), (1, 0, 8), (1, 10, 4), (1, 10, 12), (-1, 10, 8)):
        with pytest.raises(_capi.AwqNativeError):
            ops.lm_head_logprobs_plan(*bad)
        assert ops.lm_head_logprobs_workspace_bytes(*bad) == 0
    # edge targets reach column 0, V - 1 and both sides of a tile edge
    tg = O.edge_targets(2 * rt + 5, 2 * vt + 17, vt)
    assert {0, 2 * vt + 16, vt - 1, vt, 2 * vt - 1, 2 * vt} <= set(tg.tolist())
    tg = O.edge_targets(5, 300, vt, ignored=(0, 2, 4))
    assert tg[0] == -1 and tg[2] == -100 and tg[4] == 300


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_built_cases_are_exact_and_hold_their_edges(dtype_name):
    rt, vt = _tiles()
    c = O.build_lattice(rt + 1, 2 * vt + 17, 72, dtype_name, True, vt)
    r = O.case_reference(c)
    z = r["z"]
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)                       # representable in fp32: equality is a fair demand
    best, twin = c["tie"]
    assert z[0, best] == z[0, twin] == z[0].max() and r["argmax"][0] == min(best, twin)     # the maximum is tied between two indices
    assert O.case_reference(c, mutant="argmax_highest_tie")["argmax"][0] == max(best, twin)
    assert torch.isnan(c["x3"][:, :2, :]).all() and not torch.isnan(c["x3"][:, 2, :]).any()
    for kind in ("all_low", "spike", "equal"):
        e = O.build_extreme(kind, dtype_name, vt)
        r = O.case_reference(e)
        z = r["z"]
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and e["V"] % vt != 0 and e["V"] > vt
        if kind == "all_low":
            assert z.max() <= -3e4
        elif kind == "spike":
            assert (z[:, vt + 3] - np.delete(z, vt + 3, axis=1).max(-1) >= 200).all()
            assert np.allclose(r["lse"], z[:, vt + 3], rtol=0, atol=1e-80) and (r["argmax"] == vt + 3).all()
        else:
            assert (z == z[:, :1]).all() and (r["argmax"] == 0).all() and np.allclose(r["lse"], z[:, 0] + math.log(e["V"]), rtol=1e-15)


def _seen(case, mutant, round_logits=False, targets="own", init=None, x_store=None):
    """does the GPU tests' check tell the mutant from the contract on this case?"""
    want = O.case_reference(case, round_logits, targets, init, None, x_store)
    got = O.case_reference(case, round_logits, targets, init, mutant, x_store)
    n_tiles = -(-case["V"] // case["vt"])
    bnd = O.bounds(want["z"], want.get("target_logit") is not None and (case["targets"] if isinstance(targets, str) else targets), 0.0, n_tiles)
    assert not O.mismatches(want, want, bnd)               # the check is not one that rejects everything
    return bool(O.mismatches({k: got[k] for k in ("logprob", "lse", "target_logit", "argmax")}, want, bnd))


@pytest.mark.parametrize("mutant", list(O.MUTANTS))
def test_each_mutant_is_rejected_by_a_case_of_the_gpu_list(mutant):
    rt, vt = _tiles()
    shapes = O.lattice_shapes(rt, vt)
    assert (2, 17, 40) in shapes or any(k % 64 for _, _, k in shapes)
    small = next(s for s in shapes if s[0] >= 2 and s[1] >= 17 and s[2] % 64 != 0 and s[0] * s[1] * s[2] < 2_000_000)
    wide = next(s for s in shapes if s[1] > vt and s[0] >= 2)                   # more than one vocabulary tile
    plain = O.build_lattice(*small, "bf16", False, vt)
    biased = O.build_lattice(*wide, "fp16", True, vt)
    low = O.build_extreme("all_low", "bf16", vt)
    # ignored rows: -1 / -100 / V at the first, a middle and the last row, NaN in their x, outputs pre-filled with -7
    T = wide[0]
    rows = O.ignored_patterns(T, wide[1])
    tg = O.edge_targets(T, wide[1], vt, ignored=rows)
    store = biased["x_store"].copy()
    for t in rows:
        store[t * biased["ldx"]: t * biased["ldx"] + biased["K"]] = np.nan
    init = {n: np.full(T, -7.0) for n in ("logprob", "lse", "target_logit", "argmax")}
    hits = {
        "v_pad_zero": lambda: _seen(low, mutant),
        "k_tail": lambda: _seen(plain, mutant),
        "max_init_zero": lambda: _seen(low, mutant),
        "no_rescale": lambda: _seen(biased, mutant),
        "bias_not_in_lse": lambda: _seen(biased, mutant) and _seen(low, mutant),
        "target_tile_off_by_one": lambda: _seen(biased, mutant),
        "round_skipped": lambda: _seen(biased, mutant, round_logits=True),
        "argmax_highest_tie": lambda: _seen(biased, mutant),
        "ignored_written": lambda: _seen(biased, mutant, targets=tg, init=init, x_store=store),
        "nan_leak": lambda: _seen(biased, mutant, targets=tg, init=init, x_store=store),
        "row_prev": lambda: _seen(plain, mutant),
        "ldx_as_k": lambda: _seen(plain, mutant),
    }
    assert set(hits) == set(O.MUTANTS) and all(len(d.split()) >= 2 for d in O.MUTANTS.values())
    assert hits[mutant](), mutant


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _capi.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    DTYPE, SHAPE, ALIGN, NULL, WORKSPACE = -3, -4, -5, -6, -7
    names = ("x", "gamma", "weight", "bias", "targets", "logprob", "lse", "target_logit", "argmax", "ws")

    def call(t=4, v=100, k=64, ldx=64, dt=1, rnd=0, mb=0, eps=1e-6, wsb=1 << 30, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        return L.awq_lm_head_logprobs(a["x"], ldx, a["gamma"], eps, a["weight"], a["bias"], a["targets"], a["logprob"], a["lse"], a["target_logit"],
                                      a["argmax"], t, v, k, dt, rnd, a["ws"], wsb, mb, None)

    for n in ("x", "weight"):
        assert call(**{n: None}) == NULL, n
    assert call(targets=None) == NULL and call(targets=None, logprob=None) == NULL and call(targets=None, target_logit=None) == NULL
    assert call(dt=2) == DTYPE and call(dt=-1) == DTYPE
    assert call(t=0) == SHAPE and call(v=0) == SHAPE and call(k=0) == SHAPE and call(k=4) == SHAPE and call(k=68, ldx=72) == SHAPE
    assert call(ldx=56) == SHAPE and call(ldx=68) == SHAPE and call(mb=-1) == SHAPE
    assert call(ldx=128) == SHAPE and call(ldx=128, gamma=None, wsb=0) == WORKSPACE      # the norm's rows are contiguous; without it a stride is fine
    for n in ("x", "weight", "gamma", "bias", "ws"):
        assert call(**{n: p + 8}) == ALIGN, n
    for n in ("targets", "logprob", "lse", "target_logit", "argmax"):
        assert call(**{n: p + 2}) == ALIGN, n
    need = L.awq_lm_head_logprobs_workspace_bytes(4, 100, 64, 1)
    assert need > 0 and call(wsb=need - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    plan = (ctypes.c_int * 4)()
    assert L.awq_lm_head_logprobs_plan(1, 10, 8, None) == NULL and L.awq_lm_head_logprobs_plan(1, 10, 9, plan) == SHAPE
    assert L.awq_lm_head_logprobs_plan(300, 1000, 8, plan) == 0 and list(plan) == [plan[0], plan[1], -(-300 // plan[0]) * -(-1000 // plan[1]), 64]

    def rows(b=3, v=10, ld=10, dt=2, logits=p, targets=p, logprob=p, lse=p, argmax=p):
        return L.awq_token_logprobs(logits, dt, ld, targets, logprob, lse, argmax, b, v, None)

    assert rows(logits=None) == NULL and rows(targets=None) == NULL and rows(dt=3) == DTYPE
    assert rows(b=0) == SHAPE and rows(v=0) == SHAPE and rows(ld=9) == SHAPE
    assert rows(logits=p + 2) == ALIGN and rows(dt=1, logits=p + 1) == ALIGN and rows(lse=p + 2) == ALIGN and rows(targets=p + 1) == ALIGN


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    x, w = torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(8, 16, dtype=torch.bfloat16)
    with pytest.raises(_capi.AwqNativeError):
        ops.lm_head_logprobs(x, w)
    with pytest.raises(ValueError):
        ops.token_logprobs(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        ops.lm_head_logprobs(x.view(-1), w)
    assert list(inspect.signature(ops.lm_head_logprobs).parameters)[:9] == ["x", "weight", "targets", "gamma", "eps", "bias", "round_logits", "ws", "want"]
    assert list(inspect.signature(ops.token_logprobs).parameters)[:2] == ["logits", "targets"]
    import llm_awq_amd
    eng = llm_awq_amd.load_engine()
    assert callable(eng.lm_head_logprobs) and callable(eng.token_logprobs)
    assert "transformers" not in inspect.getsource(evaluate)      # perplexity_hf takes the model as an object: nothing to import


class _StubHead:
    """LMHead.logprobs on the CPU in float64: logits = h W^T, rounded to bf16 with round_logits"""

    def __init__(self, w):
        self.w = w

    def logits(self, h, round_logits):
        z = h.double() @ self.w.double().T
        return z.to(torch.bfloat16).double() if round_logits else z

    def logprobs(self, h, targets, round_logits=False, want=("logprob", "lse")):
        z = self.logits(h, round_logits)
        lp = torch.log_softmax(z, -1)
        return {"logprob": lp.gather(1, targets.long()[:, None])[:, 0], "lse": torch.logsumexp(z, -1), "argmax": z.argmax(-1).int()}


@pytest.mark.parametrize("n_tokens,seqlen", [(3 * 16 + 5, 16), (16, 16), (2 * 16 + 15, 16), (65, 64)])
def test_perplexity_window_arithmetic_is_entry_py(n_tokens, seqlen):
    g = torch.Generator().manual_seed(n_tokens)
    V, K = 50, 8
    table = torch.randn(V, K, generator=g).to(torch.bfloat16)
    head = _StubHead((torch.randn(V, K, generator=g) * 0.5).to(torch.bfloat16))
    ids = torch.randint(0, V, (1, n_tokens), generator=g)
    hidden_fn = lambda b: table[b]
    for rnd in (True, False):
        want = O.entry_py_perplexity(lambda b: head.logits(table[b[0]], rnd)[None], ids, seqlen)
        got = evaluate.perplexity(hidden_fn, head, ids, seqlen=seqlen, round_logits=rnd)
        nsamples = n_tokens // seqlen
        # the windows' NLLs are summed in fp32: seqlen - 1 + nsamples additions and a handful of single operations, each within 2^-24 relative
        assert abs(math.log(got) - math.log(want)) <= (seqlen + nsamples + 8) * 2.0 ** -24 * math.log(want)
        assert evaluate.perplexity(hidden_fn, head, ids[0], seqlen=seqlen, round_logits=rnd) == got      # [N] or [1, N]
    # the remainder is dropped: the tokens past the last whole window do not matter
    if n_tokens % seqlen:
        ids2 = ids.clone()
        ids2[0, (n_tokens // seqlen) * seqlen:] = 0
        assert evaluate.perplexity(hidden_fn, head, ids2, seqlen=seqlen) == evaluate.perplexity(hidden_fn, head, ids, seqlen=seqlen)
    with pytest.raises(ValueError):
        evaluate.perplexity(hidden_fn, head, ids[:, :seqlen - 1], seqlen=seqlen)
    # loglikelihood: the continuation's log-probs given everything before, and whether each was the greedy token
    ctx, cont = ids[0, :5], ids[0, 5:9]
    z = head.logits(table[ids[0, :8]], True)
    lp = torch.log_softmax(z, -1)[4:8]
    s, greedy = evaluate.loglikelihood(hidden_fn, head, ctx, cont)
    assert abs(s - float(lp.gather(1, cont[:, None]).sum())) < 1e-9 and greedy == bool((z[4:8].argmax(-1) == cont).all())
    # a greedy continuation, built step by step, is greedy; one changed token is not
    cur = ids[0, :5].clone()
    for _ in range(3):
        nxt = head.logits(table[cur], True)[-1].argmax()
        cur = torch.cat([cur, nxt[None]])
    assert evaluate.loglikelihood(hidden_fn, head, cur[:5], cur[5:])[1] is True
    wrong = cur[5:].clone()
    wrong[1] = (wrong[1] + 1) % V
    assert evaluate.loglikelihood(hidden_fn, head, cur[:5], wrong)[1] is False
