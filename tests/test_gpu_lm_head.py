"""gpu: the LM head (awq_lm_head, ops.lm_head, LMHead) and the token embedding gather (awq_embed_tokens) against the float64 oracle of the contract
(tests/lm_head_oracle.py): exact on the integer lattice, fused norm = unfused norm in every bit, random inputs under the derived bound, independence
of the launch shape, inactive rows, determinism, one real vocabulary, the embedding, and the closed decode step embed -> norm -> LM head -> sample
captured as one graph."""
import functools

import numpy as np
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from llm_awq_amd.lm_head import LMHead, TokenEmbedding
from llm_awq_amd.sampling import DeviceSampler
from tests import lm_head_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run_lattice(case, **kw):
    x = _dev(case["x3"])[:, -1, :]          # a strided view: row stride 3 K, the other tokens are NaN
    assert not x.is_contiguous() or case["M"] == 1
    w, bias = _dev(case["w"]), _dev(case["bias"])
    T = O.DTYPES[case["dtype_name"]]
    got32 = ops.lm_head(x, w, bias=bias, **kw)
    gotT = ops.lm_head(x, w, bias=bias, out_dtype=T, **kw)
    assert got32.dtype == torch.float32 and gotT.dtype == T
    return O.f64(got32), O.f64(gotT)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", O.LATTICE_SHAPES, ids=lambda s: "m%d-v%d-k%d" % s)
def test_lattice_rows_are_exact(shape, dtype_name, with_bias):
    """no tolerance and no exclusions: every partial sum is exact in fp32, so the fp32 output EQUALS the float64 oracle and the T output its
    nearest-even rounding (row 0 holds planted ties)"""
    case = O.build_lattice(*shape, dtype_name, with_bias)
    got32, gotT = _run_lattice(case)
    assert np.array_equal(got32, case["y_f32"])
    assert np.array_equal(gotT, case["y_T"])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_lattice_blocks_that_walk_several_tiles(dtype_name):
    """a V from the plan: with the grid forced to 2 and with the plan's own grid some block walks at least two tiles, and the last tile is partial"""
    V = O.planned_v(ops.lm_head_plan)
    p = ops.lm_head_plan(2, V, 64)
    assert -(-V // p["tile_rows"]) > p["blocks"] and V % p["tile_rows"] != 0
    case = O.build_lattice(2, V, 64, dtype_name, True)
    for mb in (2, 0):
        got32, gotT = _run_lattice(case, max_blocks=mb)
        assert np.array_equal(got32, case["y_f32"]) and np.array_equal(gotT, case["y_T"]), mb


@pytest.mark.parametrize("eps", O.EPS)
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", O.NORM_SHAPES, ids=lambda s: "m%d-v%d-k%d" % s)
def test_fused_norm_equals_unfused_norm_bit_for_bit(shape, dtype_name, eps):
    """rows whose sum of squares is exact in fp32 in any order (row 0 with a variance of the order of eps): the launch with gamma equals
    ops.rmsnorm followed by the launch without, in every bit"""
    case = O.build_norm_lattice(*shape, dtype_name, eps)
    x, g, w = _dev(case["x"]), _dev(case["gamma"]), _dev(case["w"])
    xn = ops.rmsnorm(x, g, eps)
    assert torch.isfinite(xn.float()).all()
    for od in (torch.float32, O.DTYPES[dtype_name]):
        fused, unfused = ops.lm_head(x, w, g, eps, out_dtype=od), ops.lm_head(xn, w, out_dtype=od)
        assert _same_bits(fused, unfused), od
    # ... and it is the oracle's norm that ops.rmsnorm computes, to within one code of T (rsqrtf is not a correctly rounded function)
    want = O.norm(O.f64(case["x"]), O.f64(case["gamma"]), eps, dtype_name)
    assert (np.abs(O.f64(xn) - want) <= O.ulp_T(want, dtype_name)).all()


@functools.lru_cache(maxsize=None)
def _random_case(M, V, K):
    """N(0, 1) activations, N(0, 0.02) weights, bf16; the float64 references are computed once and shared"""
    g = torch.Generator().manual_seed(M + V + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * 0.02).to(torch.bfloat16)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    bias = (torch.randn(V, generator=g) * 0.1).to(torch.bfloat16)
    dx, dw, dg, db = _dev(x), _dev(w), _dev(gamma), _dev(bias)
    xn = ops.rmsnorm(dx, dg, 1e-5)         # step 1's T values, from the kernel the fused launch equals bit for bit (tested above)
    refs = {}
    for norm, rows in ((False, x), (True, xn)):
        for out in ("f32", "T"):
            refs[norm, out] = O.reference(O.f64(rows), K, M, O.f64(w), O.f64(bias), out=out, dtype_name="bf16")
    return dx, dw, dg, db, refs


@pytest.mark.parametrize("out", ["f32", "T"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("shape", O.RANDOM_SHAPES, ids=lambda s: "m%d-v%d-k%d" % s)
def test_random_inputs_are_within_the_derived_bound(shape, norm, out):
    M, V, K = shape
    dx, dw, dg, db, refs = _random_case(*shape)
    want, absdot = refs[norm, out]
    got = O.f64(ops.lm_head(dx, dw, dg if norm else None, 1e-5, bias=db, out_dtype=torch.float32 if out == "f32" else torch.bfloat16))
    # for T output the float64 sum is the centre: the stored value is within half a code of the fp32 sum, which is within the bound of it
    centre = refs[norm, "f32"][0]
    err, lim = np.abs(got - centre), O.bound(absdot, K, out, "bf16", centre)
    print("max error / bound", float((err / lim).max()), "bound / |y| median", float(np.median(lim / np.maximum(np.abs(centre), 1e-30))))
    assert got.shape == (M, V) and np.isfinite(got).all() and (err <= lim).all()          # every element, none left out
    assert want.shape == got.shape


def test_bits_do_not_depend_on_the_launch_shape():
    """step 2's order rule: the same case at max_blocks 1, 3 and 0 gives the same bits, with gamma and without, and each row run alone equals its
    row in the M = 17 launch"""
    M, V, K = 17, 1025, 1032
    g = torch.Generator().manual_seed(5)
    x = _dev(torch.randn(M, K, generator=g).to(torch.float16))
    w = _dev((torch.randn(V, K, generator=g) * 0.02).to(torch.float16))
    gamma = _dev((1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.float16))
    for gm in (None, gamma):
        base = ops.lm_head(x, w, gm, 1e-6)
        for mb in (1, 3):
            assert _same_bits(ops.lm_head(x, w, gm, 1e-6, max_blocks=mb), base), mb
        for b in range(M):
            assert _same_bits(ops.lm_head(x[b:b + 1], w, gm, 1e-6)[0], base[b]), b
    # whether gamma is given does not change the product's order either: the fused launch is the plain launch on the normalised rows
    assert _same_bits(ops.lm_head(ops.rmsnorm(x, gamma, 1e-6), w), ops.lm_head(x, w, gamma, 1e-6))


@pytest.mark.parametrize("M", [5, 33])
def test_inactive_rows_are_left_untouched(M):
    V, K = 130, 136
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = _dev((torch.randn(V, K, generator=g) * 0.02).to(torch.bfloat16))
    gamma = _dev(torch.ones(K, dtype=torch.bfloat16))
    full = ops.lm_head(_dev(x), w, gamma, 1e-5)
    for seq in O.inactive_patterns(M):
        xs = x.clone()
        xs[torch.from_numpy(seq < 0)] = float("nan")                                     # an inactive row may hold anything
        for od in (torch.float32, torch.bfloat16):
            out = torch.full((M, V), -7.0, dtype=od, device=DEV)
            ret = ops.lm_head(_dev(xs), w, gamma, 1e-5, seqlens=_dev(seq), out=out, out_dtype=od)
            assert ret is out
            act = _dev(seq >= 0)
            assert (out[~act] == -7.0).all()                           # the sentinel is still there
            want = full if od == torch.float32 else ops.lm_head(_dev(x), w, gamma, 1e-5, out_dtype=od)
            assert _same_bits(out[act], want[act])                     # active rows: the launch without seqlens
        fresh = ops.lm_head(_dev(xs), w, gamma, 1e-5, seqlens=_dev(seq))
        assert (fresh[_dev(seq < 0)] == 0).all() and torch.isfinite(fresh).all()     # a fresh output reads as zeros there
    out = torch.full((M, V), -7.0, device=DEV)
    ops.lm_head(_dev(torch.full((M, K), float("nan"), dtype=torch.bfloat16)), w, gamma, 1e-5, seqlens=_dev(np.full(M, -1, np.int32)), out=out)
    assert (out == -7.0).all()                                         # every row inactive: the whole output untouched


def test_three_runs_give_the_same_bits():
    dx, dw, dg, db, _ = _random_case(*O.RANDOM_SHAPES[1])
    a, b, c = (ops.lm_head(dx, dw, dg, 1e-5, bias=db) for _ in range(3))
    assert _same_bits(a, b) and _same_bits(a, c)


@pytest.fixture(scope="module")
def real_weights():
    V, K = 128256, 4096
    g = torch.Generator(device=DEV).manual_seed(17)
    w = torch.empty(V, K, dtype=torch.bfloat16, device=DEV).normal_(0.0, 0.02, generator=g)
    gamma = (1.0 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(torch.bfloat16)
    x = torch.randn(8, K, device=DEV, generator=g).to(torch.bfloat16)
    xn = ops.rmsnorm(x, gamma, 1e-5)
    w[40] = (xn[0].float() * 0.01).to(torch.bfloat16)          # row 0's largest logit by far (0.01 |xn|^2 ~ 41), inside the checked rows
    idx = torch.cat([torch.arange(64, device=DEV), torch.arange(V - 64, V, device=DEV),
                     torch.randint(64, V - 64, (4096,), device=DEV, generator=g)])
    wd = w[idx].double()
    ref = xn.double() @ wd.T
    absdot = xn.double().abs() @ wd.abs().T
    yield dict(V=V, K=K, w=w, gamma=gamma, x=x, idx=idx, ref=ref, absdot=absdot)
    del w, wd


@pytest.mark.parametrize("M", [1, 8])
def test_one_real_vocabulary(real_weights, M):
    """V 128256, K 4096, bf16: checked on the device against a float64 matmul over the first 64, the last 64 and 4096 random vocabulary rows, under
    the derived bound; greedy through ops.sample_logits is the float64 argmax whenever that lies among the checked rows"""
    r = real_weights
    logits = ops.lm_head(r["x"][:M], r["w"], r["gamma"], 1e-5)
    assert logits.shape == (M, r["V"]) and logits.dtype == torch.float32
    got = logits[:, r["idx"]].double()
    lim = (r["K"] + 1) * 2.0 ** -24 * r["absdot"][:M]
    err = (got - r["ref"][:M]).abs()
    print("max error / bound", float((err / lim).max()))
    assert torch.isfinite(logits).all() and (err <= lim).all()
    tokens = ops.sample_logits(logits, torch.full((M,), 0.5, device=DEV)).cpu().tolist()
    assert tokens[0] == 40
    idx = r["idx"].cpu().tolist()
    best = r["ref"][:M].argmax(dim=1).cpu().tolist()
    for b in range(M):
        if tokens[b] in idx:
            assert tokens[b] == idx[best[b]], b
    if M == 8:                                                  # the same rows whatever the batch
        assert _same_bits(ops.lm_head(r["x"][:1], r["w"], r["gamma"], 1e-5)[0], logits[0])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("K", [8, 72, 4096])
def test_embedding_gathers_rows_and_gives_zeros_outside_the_table(K, n, dtype_name):
    V, T = 50, O.DTYPES[dtype_name]
    g = torch.Generator().manual_seed(K + n)
    table = torch.randn(V, K, generator=g).to(T)
    valid = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
    named = torch.zeros(V, dtype=torch.bool)
    named[valid.long()] = True
    table[~named] = float("nan")                                # a row no id names is never read into the result
    dt = _dev(table)
    got = ops.embed_tokens(_dev(valid), dt)
    assert got.shape == (n, K) and _same_bits(got, dt[valid.long().to(DEV)])
    for bad in (-1, V, 2 ** 31 - 1, -2 ** 31):
        tok = valid.clone()
        tok[n // 2] = bad
        got = ops.embed_tokens(_dev(tok), dt)
        want = O.embed_reference(tok.numpy(), table.float().numpy())
        assert (got[n // 2] == 0).all() and np.array_equal(got.float().cpu().numpy(), want)
    assert ops.embed_tokens(_dev(valid).view(n, 1), dt).shape == (n, 1, K)


def test_module_and_engine_binding_are_the_same_entries():
    M, V, K = 7, 127, 72
    g = torch.Generator().manual_seed(2)
    lin = torch.nn.Linear(K, V, bias=True, dtype=torch.bfloat16, device=DEV)
    norm = torch.nn.Module()
    norm.weight = torch.nn.Parameter(_dev((1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)))
    norm.variance_epsilon = 1e-5
    head = LMHead.from_modules(norm, lin)
    assert head.weight.data_ptr() == lin.weight.data_ptr() and head.norm_weight.data_ptr() == norm.weight.data_ptr()
    assert head.bias.data_ptr() == lin.bias.data_ptr()
    h = _dev(torch.randn(M, 3, K, generator=g).to(torch.bfloat16))
    seq = _dev(np.array([3, -1, 5, 6, 7, 8, -1], np.int32))
    with torch.no_grad():
        want = ops.lm_head(h[:, -1, :], lin.weight, norm.weight, 1e-5, bias=lin.bias, seqlens=seq)
        assert _same_bits(head(h, seq), want) and _same_bits(head(h[:, -1, :].contiguous(), seq), want)
        eng = llm_awq_amd.load_engine()
        assert _same_bits(eng.lm_head(h[:, -1, :], lin.weight, norm.weight, 1e-5, lin.bias, seq), want)
        assert _same_bits(eng.lm_head(h[:, -1, :], lin.weight, gamma=norm.weight, eps=1e-5, bias=lin.bias, out_dtype=torch.bfloat16, max_blocks=1),
                          ops.lm_head(h[:, -1, :], lin.weight, norm.weight, 1e-5, bias=lin.bias, out_dtype=torch.bfloat16))
        tok = _dev(torch.tensor([3, -1, 126, 127], dtype=torch.int32))
        assert _same_bits(eng.embed_tokens(tok, lin.weight), ops.embed_tokens(tok, lin.weight))
        assert _same_bits(TokenEmbedding.from_module(lin)(tok), ops.embed_tokens(tok, lin.weight))
        with pytest.raises(RuntimeError):
            eng.lm_head(h[:, -1, :], lin.weight[:, :64])


def test_the_closed_step_replays_as_one_graph():
    """embed -> (one rmsnorm standing in for the blocks) -> LM head -> DeviceSampler, whose tokens feed the next step's embedding: eight steps
    captured as one graph and replayed twice from restored state equal the eager run.  Slot 0 is inactive from the start; slot 1 meets the stop id
    in step 3 -- planted as a spike in the stop id's weight row along slot 1's step-3 activations (a bias spike would act on every slot and step
    alike) -- after which its logits row no longer changes and its token is -1."""
    B, V, K, steps, stop = 4, 1025, 136, 8, 1024
    g = torch.Generator().manual_seed(9)
    table = _dev(torch.randn(V, K, generator=g).to(torch.bfloat16))
    w = _dev((torch.randn(V, K, generator=g) * 0.02).to(torch.bfloat16))
    bias = _dev((torch.randn(V, generator=g) * 0.05).to(torch.bfloat16))
    g1 = _dev((1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16))
    g2 = _dev((1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16))
    head, embed = LMHead(w, g2, 1e-5, bias), TokenEmbedding(table)
    init = dict(tokens=torch.tensor([-1, 17, 900, 33], dtype=torch.int32), seqlens=torch.tensor([-1, 3, 7, 2], dtype=torch.int32),
                logits=torch.zeros(B, V))
    state = {k: _dev(v.clone()) for k, v in init.items()}
    u = _dev(torch.full((B,), 0.5))

    def make_sampler(stop_ids):
        smp = DeviceSampler(B, V, DEV, max_history=16, stop_ids=stop_ids)
        for b in range(B):
            smp.set_row(b, temperature=0.0)                     # greedy: the run is decided by the logits alone
        return smp

    def step(smp):
        h = ops.rmsnorm(embed(state["tokens"]), g1, 1e-5)
        head(h, state["seqlens"], out=state["logits"])
        tok = smp(state["logits"], seqlens=state["seqlens"], u=u)
        state["tokens"].copy_(tok)
        return tok, state["logits"].clone()

    # slot 1's activations going into step 3, from two steps without any stop id
    probe = make_sampler([])
    for _ in range(2):
        step(probe)
    t_in = int(state["tokens"][1])
    assert t_in >= 0
    xn = ops.rmsnorm(ops.rmsnorm(table[t_in:t_in + 1], g1, 1e-5), g2, 1e-5)
    w[stop] = (xn[0].float() * 0.02).to(torch.bfloat16)          # logit 0.02 |xn|^2 ~ 2.7 for that input (the others reach ~0.8); one more random row elsewhere

    smp = make_sampler([stop])
    sinit = {k: getattr(smp, k).clone() for k in ("history", "hist_len", "finished")}

    def reset():
        for k, v in init.items():
            state[k].copy_(v)
        for k, v in sinit.items():
            getattr(smp, k).copy_(v)

    def run():
        outs = [step(smp) for _ in range(steps)]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])

    def snapshot():
        return {**{k: v.cpu().clone() for k, v in state.items()}, **{k: getattr(smp, k).cpu().clone() for k in sinit}}

    reset()
    toks, logs = run()
    eager_t, eager_l, want = toks.cpu(), logs.cpu(), snapshot()
    assert (eager_t[:, 0] == -1).all() and (eager_l[:, 0] == 0).all()                      # never active: its logits row is never written
    assert eager_t[2, 1] == stop and (eager_t[:2, 1] >= 0).all() and (eager_t[3:, 1] == -1).all()
    assert all(torch.equal(eager_l[s, 1], eager_l[2, 1]) for s in range(3, steps))         # finished: the row no longer changes
    assert want["finished"].tolist() == [0, 1, 0, 0] and want["seqlens"].tolist() == [-1, -1, 7 + steps, 2 + steps]
    assert (eager_t[:, 2:] >= 0).all() and want["hist_len"].tolist() == [0, 3, steps, steps]
    assert want["history"][1, :3].tolist() == eager_t[:3, 1].tolist() and want["history"][2, :steps].tolist() == eager_t[:, 2].tolist()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        reset()
        run()
    torch.cuda.current_stream().wait_stream(s)
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        toks, logs = run()
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(toks.cpu(), eager_t) and torch.equal(logs.cpu(), eager_l)
        got = snapshot()
        for k, v in want.items():
            assert torch.equal(got[k], v), k
