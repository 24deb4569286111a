"""gpu: token log-probabilities (awq_lm_head_logprobs, awq_token_logprobs, ops / LMHead.logprobs / evaluate) against the float64 oracle of the
contract (tests/lm_logprobs_oracle.py): target logit and argmax exact on the integer lattice, lse and logprob within the derived bound, the ends of
the range, random rows, the same bits wherever a row is served, ignored rows, a weight matrix of more than 2^31 bytes, the companion for logits that
already exist, and the evaluate layer (perplexity, loglikelihood, one captured call)."""
import functools
import math

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import evaluate, ops
from llm_awq_amd.lm_head import LMHead
from tests import lm_head_oracle as H
from tests import lm_logprobs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("logprob", "lse", "target_logit", "argmax")
_PLAN = ops.lm_head_logprobs_plan(1, 1, 8)          # host only
RT, VT = _PLAN["row_tile"], _PLAN["vocab_tile"]
SHAPES = O.lattice_shapes(RT, VT)


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _np(res):
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def _same_bits(a, b):
    return all(a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)


def _tiles(V):
    return -(-V // VT)


def _run_case(case, round_logits=False, targets="own", fill=None, x3=None, **kw):
    x = _dev(case["x3"] if x3 is None else x3)[:, 2, :]          # a strided view: row stride 3 K, the other tokens are NaN
    assert not x.is_contiguous() or case["T"] == 1
    tg = case["targets"] if isinstance(targets, str) else targets
    want = ALL if tg is not None else ("lse", "argmax")
    out = None if fill is None else {n: torch.full((case["T"],), fill, dtype=torch.int32 if n == "argmax" else torch.float32, device=DEV) for n in want}
    res = ops.lm_head_logprobs(x, _dev(case["w"]), _dev(tg), bias=_dev(case["bias"]), round_logits=round_logits, want=want, out=out, **kw)
    assert all(res[n].dtype == (torch.int32 if n == "argmax" else torch.float32) and res[n].shape == (case["T"],) for n in want)
    return _np(res)


@pytest.mark.parametrize("round_logits", [False, True], ids=["f32", "rounded"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "t%d-v%d-k%d" % s)
def test_lattice_rows_target_logit_and_argmax_exact_lse_within_the_bound(shape, dtype_name, with_bias, round_logits):
    case = O.build_lattice(*shape, dtype_name, with_bias, VT)
    want = O.case_reference(case, round_logits)
    bnd = O.bounds(want["z"], case["targets"], 0.0, _tiles(case["V"]))
    assert (bnd["target_logit"] == 0).all()                      # the lattice: equality
    got = _run_case(case, round_logits)
    assert not O.mismatches(got, want, bnd)
    if round_logits:
        assert np.array_equal(H.round_T(got["target_logit"].astype(np.float64), dtype_name), got["target_logit"])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["all_low", "spike", "equal"])
def test_the_ends_of_the_range(kind, dtype_name):
    case = O.build_extreme(kind, dtype_name, VT)
    want = O.case_reference(case)
    bnd = O.bounds(want["z"], case["targets"], 0.0, _tiles(case["V"]))
    got = _run_case(case)
    assert not O.mismatches(got, want, bnd)
    z = want["z"]
    if kind == "all_low":
        assert z.max() <= -3e4 and np.isfinite(got["lse"]).all() and (got["lse"] < -3e4 + 10).all()
    elif kind == "spike":
        assert (np.abs(got["lse"] - z[:, VT + 3]) <= bnd["lse"]).all() and (got["argmax"] == VT + 3).all()
    else:
        assert (np.abs(got["lse"] - (z[:, 0] + math.log(case["V"]))) <= bnd["lse"]).all() and (got["argmax"] == 0).all()


@functools.lru_cache(maxsize=None)
def _random_case(T, V, K, norm):
    """N(0, 1) activations, N(0, 0.02) weights, a bias; the float64 logits are computed ONCE per shape (xn comes from ops.rmsnorm: its bits are what
    the fused call must reproduce, and rsqrtf is no function one can restate)"""
    g = torch.Generator().manual_seed(T + V + K)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * 0.02).to(torch.bfloat16)
    bias = (torch.randn(V, generator=g) * 0.05).to(torch.bfloat16)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    tg = torch.randint(0, V, (T,), generator=g).int()
    tg[3], tg[T - 1] = -100, V - 1
    xn = ops.rmsnorm(_dev(x), _dev(gamma), 1e-5).cpu() if norm else x
    ref = O.reference(H.f64(xn).reshape(-1), K, T, H.f64(w), H.f64(bias), tg.numpy(), False, "bf16", lattice=False)
    return dict(x=x, w=w, bias=bias, gamma=gamma, targets=tg, xn=xn, ref=ref, T=T, V=V, K=K)


@pytest.mark.parametrize("round_logits", [False, True], ids=["f32", "rounded"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("shape", [(130, 2000, 4096), (300, 513, 8192)], ids=lambda s: "t%d-v%d-k%d" % s)
def test_random_rows_are_within_the_derived_bound(shape, norm, round_logits):
    c = _random_case(*shape, norm)
    want = c["ref"]
    b = O.general_logit_bound(want, c["K"], "bf16", round_logits)        # (K + 1) 2^-24 (sum |xn w| + |bias|), + ulp_T / 2 under round_logits
    bnd = O.bounds(want["z"], c["targets"].numpy(), b, _tiles(c["V"]))
    kw = dict(bias=_dev(c["bias"]), round_logits=round_logits, want=ALL)
    res = ops.lm_head_logprobs(_dev(c["x"]), _dev(c["w"]), _dev(c["targets"]), gamma=_dev(c["gamma"]) if norm else None, eps=1e-5, **kw)
    assert not O.mismatches(_np(res), want, bnd, logit_bound=b)         # (two logits closer than their bounds may swap in the argmax)
    if norm:    # the fused call = ops.rmsnorm + the plain call, in every bit
        assert _same_bits(res, ops.lm_head_logprobs(_dev(c["xn"]), _dev(c["w"]), _dev(c["targets"]), **kw))


def test_a_row_has_the_same_bits_wherever_it_is_served():
    c = _random_case(130, 2000, 4096, False)
    x, w, bias, tg = _dev(c["x"]), _dev(c["w"]), _dev(c["bias"]), _dev(c["targets"])
    for rnd in (False, True):
        full = ops.lm_head_logprobs(x, w, tg, bias=bias, round_logits=rnd, want=ALL)
        alone = ops.lm_head_logprobs(x[77:78], w, tg[77:78], bias=bias, round_logits=rnd, want=ALL)
        assert _same_bits({k: v[77:78] for k, v in full.items()}, alone)
        for mb in (1, 3, 17):                                            # a capped grid walks the same tiles
            assert _same_bits(ops.lm_head_logprobs(x, w, tg, bias=bias, round_logits=rnd, want=ALL, max_blocks=mb), full)
        assert _same_bits(ops.lm_head_logprobs(x[77:78], w, tg[77:78], bias=bias, round_logits=rnd, want=ALL, max_blocks=2), alone)
        for _ in range(2):                                               # three runs
            assert _same_bits(ops.lm_head_logprobs(x, w, tg, bias=bias, round_logits=rnd, want=ALL), full)
    # the row among OTHER rows: its neighbours replaced, and moved to another place in its tile and to another tile
    x2 = torch.randn_like(x)
    x2[5], x2[129] = x[77], x[77]
    tg2 = tg.clone()
    tg2[5], tg2[129] = tg[77], tg[77]
    other = ops.lm_head_logprobs(x2, w, tg2, bias=bias, want=ALL)
    full = ops.lm_head_logprobs(x, w, tg, bias=bias, want=ALL)
    for r in (5, 129):
        assert _same_bits({k: v[r:r + 1] for k, v in other.items()}, {k: v[77:78] for k, v in full.items()})


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_ignored_rows_keep_what_they_held_and_leak_nothing(dtype_name):
    T, V, K = RT + 5, 2 * VT + 17, 72
    case = O.build_lattice(T, V, K, dtype_name, True, VT)
    rows = O.ignored_patterns(T, V)
    assert rows == [0, T // 2, T - 1]
    tg = O.edge_targets(T, V, VT, ignored=rows)
    assert [int(tg[r]) for r in rows] == [-1, -100, V]
    x3 = case["x3"].clone()
    x3[rows] = float("nan")                                              # NaN in the ignored rows of x
    store = H.f64(x3).reshape(-1)[2 * K:]
    init = {n: np.full(T, -7.0) for n in ALL}
    want = O.case_reference(case, targets=tg, init=init, x_store=store)
    bnd = O.bounds(want["z"], tg, 0.0, _tiles(V))
    got = _run_case(case, targets=tg, fill=-7, x3=x3)
    assert not O.mismatches(got, want, bnd)
    for n in ALL:
        assert (got[n][rows] == -7).all()
    assert not (got["argmax"][[r for r in range(T) if r not in rows]] == -7).any()
    # every row ignored: nothing is written (and nothing read: the weights may hold anything)
    none = np.array([(-1, -100, V)[t % 3] for t in range(T)], dtype=np.int32)
    got = _run_case(dict(case, w=torch.full_like(case["w"], float("nan"))), targets=none, fill=-7, x3=x3)
    assert all((got[n] == -7).all() for n in ALL)
    # fresh outputs are zero-filled
    res = _np(ops.lm_head_logprobs(_dev(x3)[:, 2, :], _dev(case["w"]), _dev(tg), bias=_dev(case["bias"]), want=ALL))
    assert all((res[n][rows] == 0).all() for n in ALL)
    # targets=None: lse and argmax for every row
    want = O.case_reference(case, targets=None)
    got = _run_case(case, targets=None, fill=-7)
    assert set(got) == {"lse", "argmax"} and not O.mismatches(got, want, O.bounds(want["z"], None, 0.0, _tiles(V)))
    with pytest.raises(ValueError):
        ops.lm_head_logprobs(_dev(x3)[:, 2, :], _dev(case["w"]), None, want=("logprob",))


def test_byte_offsets_of_the_llama3_matrix():
    """(3, 128256, 4096) bf16: the 1.05 GB matrix of Llama-3.  The rows' dominant logits and targets sit in the LAST vocabulary rows, whose offsets are
    the largest the shape has (1.05e9 bytes: below 2^31 -- the next test crosses it).  The oracle's product is taken in vocabulary chunks."""
    T, V, K = 3, 128256, 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    w = (torch.randn(V, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
    top = [V - 1, V - 2 * VT, V - VT - 1]
    for t, v in enumerate(top):
        w[v] = (x[t].float() * 0.01).to(torch.bfloat16)                  # logit 0.01 |x|^2 ~ 41: far above the N(0, 1.28) crowd
    tg = torch.tensor(top, dtype=torch.int32)
    res = _np(ops.lm_head_logprobs(x, w, _dev(tg), want=ALL))
    xd = x.cpu().double()
    z, absdot = np.empty((T, V)), np.empty((T, V))
    wc = w.cpu()
    for v0 in range(0, V, 16384):
        blk = wc[v0:v0 + 16384].double()
        z[:, v0:v0 + 16384] = (xd @ blk.T).numpy()
        absdot[:, v0:v0 + 16384] = (xd.abs() @ blk.abs().T).numpy()
    want = O.from_logits(z, tg.numpy())
    want["z"] = z
    bnd = O.bounds(z, tg.numpy(), H.bound(absdot, K), _tiles(V))
    assert not O.mismatches(res, want, bnd, logit_bound=H.bound(absdot, K)) and res["argmax"].tolist() == top and (want["logprob"] > -1e-3).all()


def test_byte_offsets_past_2_to_the_31():
    """a weight matrix of 2.16e9 bytes: zero everywhere (logit 0: exp(0) = 1 each, known without a product) but for a few hundred rows, the dominant
    ones and the targets among those whose byte offset exceeds 2^31"""
    T, V, K = 3, 132000, 8200
    first_past = -(-2 ** 31 // (2 * K))
    assert V * K * 2 > 2 ** 31 and first_past < V - 2 * VT
    g = torch.Generator().manual_seed(6)
    w = torch.zeros(V, K, dtype=torch.bfloat16, device=DEV)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    live = sorted(set(range(first_past - 3, first_past + 3)) | set(range(V - 300, V)) | {0, 1, VT, 70000})
    wl = (torch.randn(len(live), K, generator=g) * 0.02).to(torch.bfloat16)
    top = [V - 1, first_past + 1, V - VT - 1]
    for t, v in enumerate(top):
        wl[live.index(v)] = (x[t].float() * 0.01).to(torch.bfloat16)
    w[torch.tensor(live, device=DEV)] = _dev(wl)
    tg = torch.tensor(top, dtype=torch.int32)
    res = _np(ops.lm_head_logprobs(_dev(x), w, _dev(tg), want=ALL))
    z, absdot = np.zeros((T, V)), np.zeros((T, V))
    z[:, live] = H.f64(x) @ H.f64(wl).T
    absdot[:, live] = np.abs(H.f64(x)) @ np.abs(H.f64(wl)).T
    want = O.from_logits(z, tg.numpy())
    want["z"] = z
    bnd = O.bounds(z, tg.numpy(), H.bound(absdot, K), _tiles(V))
    assert not O.mismatches(res, want, bnd, logit_bound=H.bound(absdot, K)) and res["argmax"].tolist() == top


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("V", [1, 1025, 128256])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_token_logprobs_on_existing_logits(B, V, dtype):
    g = torch.Generator().manual_seed(B + V)
    store = (torch.randn(B, V + 24, generator=g) * 3.0).to(dtype)
    store[:, V:] = float("nan")                                          # beyond the row: never read
    if V > 2:
        store[0, 1], store[0, V - 1] = 30.0, 30.0                        # a tied maximum: the lowest index wins
        store[B - 1, :V] -= 120.0                                         # a row far below zero
    logits = _dev(store)[:, :V]                                           # row stride V + 24
    tg = torch.randint(0, V, (B,), generator=g).int()
    if B > 1:
        tg[1] = -1
    tg[0] = V - 1
    z = H.f64(store[:, :V])
    for targets in (tg, None):
        init = {n: np.full(B, -7.0) for n in ALL}
        want = O.from_logits(z, None if targets is None else targets.numpy(), init)
        bnd = O.bounds(z, None if targets is None else targets.numpy(), 0.0, n_tiles=1, levels=O.LEVELS_ROWS)   # the logits are given: a zero logit term
        names = ("logprob", "lse", "argmax") if targets is not None else ("lse", "argmax")
        out = {n: torch.full((B,), -7, dtype=torch.int32 if n == "argmax" else torch.float32, device=DEV) for n in names}
        got = _np(ops.token_logprobs(logits, _dev(targets), out=out))
        assert set(got) == set(names) and not O.mismatches(got, want, bnd)
    if V > 2:
        assert got["argmax"][0] == 1


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_token_logprobs_of_the_lm_heads_own_logits_agrees_with_the_fused_call(dtype_name):
    T, V, K = 33, 2 * VT + 17, 136
    case = O.build_lattice(T, V, K, dtype_name, True, VT)
    x, w, bias, tg = _dev(case["x3"])[:, 2, :], _dev(case["w"]), _dev(case["bias"]), _dev(case["targets"])
    fused = _np(ops.lm_head_logprobs(x, w, tg, bias=bias, want=ALL))
    logits = ops.lm_head(x, w, bias=bias)                                # fp32 [T, V], as the sampler is fed
    rows = _np(ops.token_logprobs(logits, tg))
    want = O.case_reference(case)
    assert np.array_equal(logits.cpu().numpy()[np.arange(T), case["targets"]], fused["target_logit"]) and np.array_equal(rows["argmax"], fused["argmax"])
    b1 = O.bounds(want["z"], case["targets"], 0.0, _tiles(V))
    b2 = O.bounds(want["z"], case["targets"], 0.0, 1, O.LEVELS_ROWS)
    assert (np.abs(rows["lse"].astype(np.float64) - fused["lse"]) <= b1["lse"] + b2["lse"]).all()
    assert not O.mismatches(rows, want, b2)


def _toy_model(V=1000, K=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * 0.3).to(torch.bfloat16)
    return table, w


def test_module_and_engine_binding_reach_the_same_entry():
    table, w = _toy_model()
    g = torch.Generator().manual_seed(4)
    gamma = _dev((1.0 + 0.1 * torch.randn(64, generator=g)).to(torch.bfloat16))
    bias = _dev((torch.randn(1000, generator=g) * 0.05).to(torch.bfloat16))
    h = _dev(torch.randn(3, 7, 64, generator=g).to(torch.bfloat16))
    tg = _dev(torch.randint(0, 1000, (3, 7), generator=g).int())
    tg[1, 2] = -100
    head = LMHead(_dev(w), gamma, 1e-5, bias)
    want = ops.lm_head_logprobs(h.reshape(21, 64), head.weight, tg.reshape(21), gamma, 1e-5, bias, True, want=ALL)
    assert _same_bits(head.logprobs(h, tg, round_logits=True, want=ALL), want)                 # [B, S, K]: every position
    assert _same_bits(head.logprobs(h.reshape(21, 64), tg.reshape(21), round_logits=True, want=ALL), want)
    eng = llm_awq_amd.load_engine()
    lp, lse, tl, am = eng.lm_head_logprobs(h.reshape(21, 64), head.weight, tg.reshape(21), gamma, 1e-5, bias, True)
    assert _same_bits({"logprob": lp, "lse": lse, "target_logit": tl, "argmax": am}, want)
    logits = ops.lm_head(h.reshape(21, 64), head.weight, gamma, 1e-5, bias)
    lp, lse, am = eng.token_logprobs(logits, tg.reshape(21))
    assert _same_bits({"logprob": lp, "lse": lse, "argmax": am}, ops.token_logprobs(logits, tg.reshape(21)))
    with pytest.raises(RuntimeError):
        eng.lm_head_logprobs(h.reshape(21, 64), head.weight[:, :32])


@pytest.mark.parametrize("round_logits", [False, True], ids=["f32", "rounded"])
def test_perplexity_of_a_toy_model_is_entry_pys_within_the_summed_bound(round_logits):
    V, K, seqlen, nsamples = 1000, 64, 64, 3
    table, w = _toy_model(V, K)
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, V, (1, nsamples * seqlen + 11), generator=g)                       # 3 windows and a remainder
    head = LMHead(_dev(w))
    dtab = _dev(table)
    got = evaluate.perplexity(lambda b: dtab[b.to(DEV)], head, ids, seqlen=seqlen, round_logits=round_logits)

    def logits_fn(batch):                                                                     # float64, rounded to bf16 as nn.Linear stores them
        z = table[batch[0]].double() @ w.double().T
        return (z.to(torch.bfloat16).double() if round_logits else z)[None]

    want = O.entry_py_perplexity(logits_fn, ids, seqlen)
    # the per-token bounds, summed as the NLLs are: sum over a window / (seqlen - 1) * seqlen, over the windows / (nsamples * seqlen)
    total = 0.0
    for i in range(nsamples):
        win = ids[0, i * seqlen:(i + 1) * seqlen]
        ref = O.reference(H.f64(table[win[:-1]]).reshape(-1), K, seqlen - 1, H.f64(w), None, win[1:].numpy(), False, "bf16", lattice=False)
        b = H.bound(ref["absdot"], K)
        if round_logits:    # both sides round to bf16: half an ulp each around logits that differ by at most b
            b = b + H.ulp_T(np.abs(ref["z"]) + b, "bf16")
        total += O.bounds(ref["z"], win[1:].numpy(), b, _tiles(V))["logprob"].sum() / (seqlen - 1) * seqlen
    slack = (seqlen + nsamples + 8) * 2.0 ** -24 * math.log(want)                             # the fp32 sums of evaluate.perplexity itself
    assert abs(math.log(got) - math.log(want)) <= total / (nsamples * seqlen) + slack
    assert 1.0 < got < V * 50


def test_loglikelihood_says_whether_the_continuation_was_greedy():
    table, w = _toy_model()
    head, dtab = LMHead(_dev(w)), _dev(table)
    hidden_fn = lambda b: dtab[b.to(DEV)]
    cur = torch.tensor([5, 17, 900, 33, 2])
    for _ in range(4):                                                                        # a greedy continuation, built step by step
        am = head.logprobs(dtab[cur[-1:].to(DEV)], None, round_logits=True, want=("argmax",))["argmax"]
        cur = torch.cat([cur, am.cpu().long()])
    s, greedy = evaluate.loglikelihood(hidden_fn, head, cur[:5], cur[5:])
    ref = O.reference(H.f64(table[cur[4:8]]).reshape(-1), 64, 4, H.f64(w), None, cur[5:].numpy(), False, "bf16", lattice=False)
    z = H.round_T(ref["z"], "bf16")                                                           # the reference's logits: rounded to bf16
    lp = O.from_logits(z, cur[5:].numpy())["logprob"]
    b = H.bound(ref["absdot"], 64)
    b = b + H.ulp_T(np.abs(ref["z"]) + b, "bf16")                                             # both sides round: half an ulp each
    assert greedy is True and abs(s - lp.sum()) <= O.bounds(z, cur[5:].numpy(), b, _tiles(1000))["logprob"].sum()
    wrong = cur[5:].clone()
    wrong[2] = (wrong[2] + 1) % 1000
    s2, greedy2 = evaluate.loglikelihood(hidden_fn, head, cur[:5], wrong)
    assert greedy2 is False and s2 < s


def test_one_call_replays_as_a_graph_after_the_targets_changed_in_place():
    T, V, K = RT + 5, 2 * VT + 17, 136
    case = O.build_lattice(T, V, K, "bf16", True, VT)
    x, w, bias = _dev(case["x3"])[:, 2, :], _dev(case["w"]), _dev(case["bias"])
    tg = _dev(case["targets"]).clone()
    ws = torch.empty(ops.lm_head_logprobs_workspace_bytes(T, V, K), dtype=torch.uint8, device=DEV)
    out = {n: torch.zeros(T, dtype=torch.int32 if n == "argmax" else torch.float32, device=DEV) for n in ALL}
    call = lambda: ops.lm_head_logprobs(x, w, tg, bias=bias, round_logits=True, ws=ws, want=ALL, out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    tg2 = np.roll(case["targets"], 3).copy()
    tg2[4] = -1
    tg.copy_(_dev(tg2))
    for n in ALL:
        out[n].fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    got = _np(out)
    eager = _np(ops.lm_head_logprobs(x, w, _dev(tg2), bias=bias, round_logits=True, want=ALL,
                                     out={n: torch.full_like(out[n], -7) for n in ALL}))
    assert all(np.array_equal(got[n], eager[n]) for n in ALL) and got["lse"][4] == -7
    want = O.case_reference(case, True, targets=tg2, init={n: np.full(T, -7.0) for n in ALL})
    assert not O.mismatches(got, want, O.bounds(want["z"], tg2, 0.0, _tiles(V)))
