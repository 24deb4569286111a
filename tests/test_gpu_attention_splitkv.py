"""Split-KV attention on the MI355X (csrc/awq_attn_splitkv_cdna4.hip): the needle cases of tests/attn_splitkv_oracle.py bit for bit under
a forced chunk of 64 keys, random inputs under the plan against the float64 oracle (tests/attn_prefill_oracle.py) with a derived
elementwise bound, agreement with the one-pass kernel, the routing of flash_attn_func, determinism, graph replay and padding."""
import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_cases as C
from tests import attn_prefill_oracle as O
from tests import attn_splitkv_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _flash():
    llm_awq_amd.install_as_flash_attn()
    from flash_attn import flash_attn_func  # the module name tinychat imports

    return flash_attn_func


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def chunk64():
    _capi.tune(attn_splitkv_chunk=S.CHUNK)
    yield
    _capi.tune(attn_splitkv_chunk=0)


# ------------------------------------------------------------------------------------------------------------------------
# needle cases: bit equality, every row, both entry points, chunk forced to 64 keys
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", S.CASES, ids=S.case_id)
def test_needle_cases_bit_exact_with_forced_chunks(spec, chunk64):
    case = C.Case(spec)
    s = case.spec
    splits, chunk = ops.attn_splitkv_plan(s["B"], s["H"], s["Hkv"], s["Dh"], s["Sq"], s["Sk"], case.causal)
    assert chunk == 64 and splits == (s["Sk"] + 63) // 64 > 1  # the split kernels run, not the one-pass one
    q, k, v = case.to(DEV)
    assert q.stride() == case.q.stride() and k.stride() == case.k.stride()
    want = case.target.view(torch.int16)
    out = ops.attn_splitkv(q, k, v, case.scale, case.causal)
    torch.cuda.synchronize()
    assert out.shape == case.target.shape and out.is_contiguous()
    assert torch.isfinite(out.float()).all()
    got = out.cpu().view(torch.int16)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())
    out2 = _flash()(q, k, v, 0.0, case.scale, case.causal)  # routed by the plan, which follows the knob
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu().view(torch.int16), want)


def test_the_one_key_last_chunk_leaves_every_row_finite_and_on_target(chunk64):
    """Sq = 8, Sk = 3 * 64 + 1: the last chunk holds one key; rows 0 .. 6 attend nothing of it (l = 0, m = -inf in their partial)."""
    for spec in [s for s in S.CASES if (s["Sq"], s["Sk"]) == (8, 193)]:
        case = C.Case(spec)
        q, k, v = case.to(DEV)
        out = ops.attn_splitkv(q, k, v, case.scale, case.causal)
        assert torch.isfinite(out.float()).all(), spec["name"]
        assert torch.equal(out.cpu().view(torch.int16), case.target.view(torch.int16)), spec["name"]


# ------------------------------------------------------------------------------------------------------------------------
# random inputs under the plan, against float64, elementwise
# ------------------------------------------------------------------------------------------------------------------------
def make(B, H, Hkv, Dh, Sq, Sk, dtype, seed, fused=False, pad=2):
    """The distributions of tests/test_gpu_attention_prefill.py::make (q ~ 1.5 N, k ~ N, v ~ 1 + 0.5 N), drawn on the GPU; with `fused`
    q, k and v are views of one qkv tensor whose rows >= Sq / >= Sk hold NaN."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (1.5 * torch.randn(B, Sq, H, Dh, generator=g, device=DEV)).to(dtype)
    k = torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV).to(dtype)
    v = (1 + 0.5 * torch.randn(B, Sk, Hkv, Dh, generator=g, device=DEV)).to(dtype)
    if fused:
        rows = max(Sq, Sk) + pad
        qkv = torch.full((B, rows, (H + 2 * Hkv) * Dh), float("nan"), dtype=dtype, device=DEV)
        qkv[:, :Sq, :H * Dh] = q.reshape(B, Sq, -1)
        qkv[:, :Sk, H * Dh:(H + Hkv) * Dh] = k.reshape(B, Sk, -1)
        qkv[:, :Sk, (H + Hkv) * Dh:] = v.reshape(B, Sk, -1)
        q = qkv[:, :Sq, :H * Dh].view(B, Sq, H, Dh)
        k = qkv[:, :Sk, H * Dh:(H + Hkv) * Dh].view(B, Sk, Hkv, Dh)
        v = qkv[:, :Sk, (H + Hkv) * Dh:].view(B, Sk, Hkv, Dh)
    return q, k, v


limit = S.bound  # the one-pass bound plus the combine term (2 splits + 60) 2^-24 A, derived in that function's docstring


RANDOM = [  # (Sq, Sk, G); the dtype / head dim mix runs over both lists below
    (1, 2048, 4), (1, 2049, 4), (4, 2111, 4), (32, 3000, 4), (1, 8193, 8),
]
_REF = {}


def _random(Sq, Sk, G, dtype, Dh):
    """Inputs and their float64 reference, computed once per case and shared by the tests below (never written to)."""
    key = (Sq, Sk, G, dtype, Dh)
    if key not in _REF:
        B, Hkv = (2, 2) if Sk < 8000 else (1, 1)
        q, k, v = make(B, G * Hkv, Hkv, Dh, Sq, Sk, dtype, seed=Sq * 31 + Sk + Dh, fused=(Sq == 4))
        ref, Aw, qk = O.attention(q, k, v, None, True, stats=True)
        _REF[key] = (q, k, v, ref, Aw, qk)
    return _REF[key]


def _mix():
    out = []
    for n, (Sq, Sk, G) in enumerate(RANDOM):
        for j, dt in enumerate((torch.float16, torch.bfloat16)):
            out.append((Sq, Sk, G, dt, (64, 128)[(n + j) % 2]))
    return out


def _check(out, ref, lim, what):
    assert torch.isfinite(out.float()).all(), what
    err = (out.double() - ref).abs()
    print(f"{what}: max err / bound = {float((err / lim).max()):.3f}")
    bad = err > lim
    assert not bad.any(), (what, int(bad.sum()), float((err / lim).max()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("Sq,Sk,G,dtype,Dh", _mix(), ids=lambda x: str(x).replace("torch.", ""))
def test_random_inputs_within_the_derived_bound_and_agree_with_the_one_pass_kernel(Sq, Sk, G, dtype, Dh):
    """Elementwise |out - float64| <= tests.attn_prefill_oracle.bound + (2 splits + 60) 2^-24 A.  The combine term (derived in
    tests.attn_splitkv_oracle.bound): the two fp32 sums over the splits, one fmaf per split each, cost splits 2^-24 relative on the
    numerator and on the denominator; a weight 2^(m_s - M) carries the rounding of its argument and one ulp of exp2, at most
    30 * 2^-24 relative for every split heavy enough to show, and since the same weight multiplies O_s and l_s only the shift of weight
    between splits counts, 2 * 30 * 2^-24 A.  Nothing here was tuned to what the kernel produces (the measured maxima are 0.5 of the bound,
    the half ulp of the final rounding)."""
    q, k, v, ref, Aw, qk = _random(Sq, Sk, G, dtype, Dh)
    B, _, H, _ = q.shape
    splits, chunk = ops.attn_splitkv_plan(B, H, H // G, Dh, Sq, Sk, True)
    assert splits > 1 and chunk >= 1024  # no knob: the plan itself splits here
    out = ops.attn_splitkv(q, k, v, None, True)
    _check(out, ref, limit(ref, Aw, qk, dtype, Sk, Dh, Dh ** -0.5, splits), f"split x{splits}")
    out_e = _engine().attn_splitkv(q, k, v, Dh ** -0.5, True)
    assert torch.equal(bits(out_e), bits(out))
    one = _engine().attn_prefill(q, k, v, Dh ** -0.5, True)  # the one-pass kernel on the same inputs: within ITS bound of the same reference
    _check(one, ref, O.bound(ref, Aw, qk, dtype, Sk, Dh, Dh ** -0.5), "one-pass")


# ------------------------------------------------------------------------------------------------------------------------
# routing
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 128), (torch.bfloat16, 64)])
def test_flash_attn_func_takes_the_split_path_where_the_plan_splits(dtype, Dh):
    q, k, v = make(1, 32, 8, Dh, 1, 4096, dtype, seed=7)
    assert ops.attn_splitkv_plan(1, 32, 8, Dh, 1, 4096, True)[0] > 1
    want = ops.attn_splitkv(q, k, v, None, True)
    assert torch.equal(bits(ops.flash_attn_func(q, k, v, None, True)), bits(want))
    assert torch.equal(bits(_flash()(q, k, v, causal=True)), bits(want))
    one = _engine().attn_prefill(q, k, v, Dh ** -0.5, True)
    ref, Aw, qk = O.attention(q, k, v, None, True, stats=True)
    _check(one, ref, O.bound(ref, Aw, qk, dtype, 4096, Dh, Dh ** -0.5), "one-pass")
    _check(want, ref, limit(ref, Aw, qk, dtype, 4096, Dh, Dh ** -0.5, ops.attn_splitkv_plan(1, 32, 8, Dh, 1, 4096, True)[0]), "split")


@pytest.mark.parametrize("Sq,Sk", [(1, 500), (130, 700)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_below_the_floor_nothing_changes(Sq, Sk, dtype):
    q, k, v = make(2, 8, 2, 128, Sq, Sk, dtype, seed=Sq + Sk, fused=True)
    assert ops.attn_splitkv_plan(2, 8, 2, 128, Sq, Sk, True)[0] == 1
    one = _engine().attn_prefill(q, k, v, 128 ** -0.5, True)
    for out in (ops.flash_attn_func(q, k, v, None, True), _flash()(q, k, v, causal=True), ops.attn_splitkv(q, k, v, None, True),
                _engine().attn_splitkv(q, k, v, 128 ** -0.5, True)):
        assert torch.equal(bits(out), bits(one))


@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128)])
def test_non_causal_split_within_the_bound(dtype, Dh):
    B, H, Hkv, Sq, Sk = 2, 8, 2, 4, 2500
    q, k, v = make(B, H, Hkv, Dh, Sq, Sk, dtype, seed=19)
    splits = ops.attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, False)[0]
    assert splits > 1
    out = _flash()(q, k, v, causal=False)
    ref, Aw, qk = O.attention(q, k, v, None, False, stats=True)
    _check(out, ref, limit(ref, Aw, qk, dtype, Sk, Dh, Dh ** -0.5, splits), "non-causal split")
    assert torch.equal(bits(out), bits(ops.attn_splitkv(q, k, v, None, False)))


def test_softmax_scale_argument_reaches_the_split_kernel():
    q, k, v = make(1, 8, 2, 128, 2, 2300, torch.bfloat16, seed=23)
    out = ops.attn_splitkv(q, k, v, 0.05, True)
    ref, Aw, qk = O.attention(q, k, v, 0.05, True, stats=True)
    _check(out, ref, limit(ref, Aw, qk, torch.bfloat16, 2300, 128, 0.05, ops.attn_splitkv_plan(1, 8, 2, 128, 2, 2300, True)[0]), "scale 0.05")
    assert torch.equal(bits(_flash()(q, k, v, softmax_scale=0.05, causal=True)), bits(out))


# ------------------------------------------------------------------------------------------------------------------------
# determinism, graph capture, padding
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,Dh", [(torch.float16, 64), (torch.bfloat16, 128)])
def test_same_call_twice_and_graph_replays_give_the_same_bits(dtype, Dh):
    q, k, v = make(1, 32, 8, Dh, 1, 4096, dtype, seed=11)
    f = _flash()
    a = f(q, k, v, causal=True)
    b = f(q, k, v, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on a side stream
        f(q, k, v, causal=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        o = f(q, k, v, causal=True)  # the workspace comes from the graph's pool
    for _ in range(2):
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(o), bits(a))
    # new keys and values in place: the replay reads them
    gen = torch.Generator(device=DEV).manual_seed(12)
    k.copy_(torch.randn(k.shape, generator=gen, device=DEV))
    v.copy_(1 + 0.5 * torch.randn(v.shape, generator=gen, device=DEV))
    want = f(q, k, v, causal=True)
    assert not torch.equal(bits(want), bits(a))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(o), bits(want))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_nan_rows_behind_the_views_do_not_reach_the_output(dtype):
    B, H, Hkv, Dh, Sq, Sk = 1, 8, 2, 128, 3, 2113  # the last tile of the last split holds one key; rows up to Sk + 63 would fill it
    q, k, v = make(B, H, Hkv, Dh, Sq, Sk, dtype, seed=29)
    kb = torch.full((B, Sk + 100, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
    vb = torch.full((B, Sk + 100, Hkv, Dh), float("nan"), dtype=dtype, device=DEV)
    kb[:, :Sk], vb[:, :Sk] = k, v
    assert ops.attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, True)[0] > 1
    want = ops.attn_splitkv(q, k, v, None, True)
    got = ops.attn_splitkv(q, kb[:, :Sk], vb[:, :Sk], None, True)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(bits(got), bits(want))
    qf, kf, vf = make(B, H, Hkv, Dh, Sq, Sk, dtype, seed=29, fused=True, pad=70)  # the same values as views of one NaN-padded qkv tensor
    assert torch.equal(bits(ops.attn_splitkv(qf, kf, vf, None, True)), bits(want))
