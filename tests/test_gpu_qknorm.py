"""The per-head q/k RMSNorm fused into the rope + KV-store launches, on the MI355X (csrc/awq_rope.hpp, the NORM instantiations of
rope_kv_store_natural_kernel and rope_kv_store_natural_fp8_kernel).

The yardstick is BIT EQUALITY with the composition the launch replaces, run on the device with the entries that exist without it: copy
the q and k heads out of qkv, `ops.rmsnorm(heads.view(-1, Dh), gamma_T, eps)`, write them back into a copy of qkv, run the plain store.
q_out, the caches or pools, the FP8 scales and guard bands around every output the test allocates are compared byte for byte.  The gammas
are T-representable there and q_gamma != k_gamma, so a swap is seen.  One case has a float32 gamma that no T holds (1 + w) and is held
against round_T of a float64 evaluation instead (tests/qknorm_oracle.py)."""
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import ops
from tests import qknorm_oracle as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(4, 2, 128, 128), (2, 1, 64, 64), (4, 2, 128, 64), (6, 2, 64, 32)]  # (H, Hkv, Dh, rot)
GUARD = 256  # bytes on either side of an output


def _engine():
    llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine

    return awq_inference_engine


class Guarded:
    """A tensor of `shape` inside a flat byte buffer with GUARD bytes on either side, every byte a position-dependent pattern, so that two
    runs that start from the same pattern can be compared whole -- what a call leaves alone stays equal too."""

    def __init__(self, shape, dtype, salt):
        n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
        self.raw = ((torch.arange(n + 2 * GUARD, device=DEV) * 37 + salt) % 251).to(torch.uint8)
        self.initial = self.raw.clone()
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)

    def initial_t(self):
        return self.initial[GUARD:-GUARD].view(self.t.dtype).view(self.t.shape)

    def guards_intact(self):
        return torch.equal(self.raw[:GUARD], self.initial[:GUARD]) and torch.equal(self.raw[-GUARD:], self.initial[-GUARD:])


def _outputs(shape4, dtype, fp8, q_shape=None):
    """caches or pools (and scales) of one run, and q_out where the caller hands one in; the same bytes every time."""
    out = dict(k=Guarded(shape4, torch.uint8 if fp8 else dtype, 1), v=Guarded(shape4, torch.uint8 if fp8 else dtype, 2))
    if fp8:
        out.update(ks=Guarded(shape4[:3], torch.float32, 3), vs=Guarded(shape4[:3], torch.float32, 4))
    if q_shape is not None:
        out.update(q=Guarded(q_shape, dtype, 5))
    return out


def _scales(o):
    return dict(k_scale=o["ks"].t, v_scale=o["vs"].t) if "ks" in o else {}


def _same(a, b):
    """Two runs' outputs, byte for byte over the whole buffers, guard bands untouched; at least the caches were written."""
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].guards_intact() and b[name].guards_intact(), name
        diff = int((a[name].raw != b[name].raw).sum())
        assert diff == 0, (name, diff)
    assert not torch.equal(a["k"].raw, a["k"].initial) and not torch.equal(a["v"].raw, a["v"].initial)


def _qbits(t):
    return t.contiguous().view(torch.int16)


def _gammas(Dh, dtype, seed):
    """T-representable, q != k, with a zero and a negative entry planted."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    qg, kg = ((1.0 + 0.3 * torch.randn(Dh, generator=g, device=DEV)).to(dtype) for _ in range(2))
    qg[3], qg[5], kg[Dh - 2], kg[9] = 0.0, -1.25, 0.0, -0.5
    assert not torch.equal(qg, kg)
    return qg, kg


def _tokens(n_tokens, H, Hkv, Dh, dtype, seed):
    """[n_tokens, (H + 2 Hkv) Dh] with the planted heads: an all-zero q head and k head, one 60000-magnitude outlier (finite in fp16),
    a head of fp16 subnormals."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n_tokens, H + 2 * Hkv, Dh, generator=g, device=DEV)
    last = n_tokens - 1  # (a decode step of the module tests brings two tokens: the third plant shares the second's row)
    x[0, 0] = 0.0
    x[0, H] = 0.0
    x[1, 1, 7] = 60000.0
    x[1, H + Hkv - 1, Dh - 1] = -60000.0
    x[min(2, last), H - 1] = torch.randn(Dh, generator=g, device=DEV) * 4e-7  # below fp16's smallest normal 6.1e-5: subnormals and zeros
    x[min(2, last), H] = torch.randn(Dh, generator=g, device=DEV) * 2e-6
    return x.to(dtype).reshape(n_tokens, -1)


def _compose(qkv, H, Hkv, Dh, qg, kg, eps):
    return Q.compose(qkv, H, Hkv, Dh, qg, kg, eps, norm=ops.rmsnorm)


def _angles(*shape, seed):
    return (30.0 * torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)).contiguous()


def _no_nan(q):
    assert not torch.isnan(q.float()).any()


# ---- host position ---------------------------------------------------------------------------------------------------------------
def _host_case(shape, dtype, fp8, eps, strided=False):
    H, Hkv, Dh, rot = shape
    B, S, start, lmax, Bc = 2, 3, 5, 16, 3
    W = (H + 2 * Hkv) * Dh
    qkv = _tokens(B * S, H, Hkv, Dh, dtype, 11).view(B, S, W)
    qg, kg = _gammas(Dh, dtype, 12)
    fr = _angles(S, B, rot, seed=13)
    composed = _compose(qkv, H, Hkv, Dh, qg, kg, eps)
    if strided:  # rows of a wider buffer: row stride W + 8, batch stride (S + 1) rows
        wide, widec = (torch.full((B, S + 1, W + 8), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
        wide[:, :S, :W], widec[:, :S, :W] = qkv, composed
        qkv, composed = wide[:, :S, :W], widec[:, :S, :W]
        assert not qkv.is_contiguous()
    store, fused_store = (ops.rope_kv_store_natural_fp8, ops.rope_kv_store_natural_fp8_qknorm) if fp8 else (ops.rope_kv_store_natural,) * 2
    a, b = _outputs((Bc, lmax, Hkv, Dh), dtype, fp8), _outputs((Bc, lmax, Hkv, Dh), dtype, fp8)
    sc = lambda o: (o["ks"].t, o["vs"].t) if fp8 else ()
    q_fused = fused_store(qkv, fr, a["k"].t, a["v"].t, *sc(a), start, H, Hkv, q_norm=qg, k_norm=kg, norm_eps=eps)
    q_want = store(composed, fr, b["k"].t, b["v"].t, *sc(b), start, H, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q_fused), _qbits(q_want))
    _same(a, b)
    _no_nan(q_fused)
    return q_fused, a


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_position_is_the_composition_bit_for_bit(shape, dtype, fp8):
    H, Hkv, Dh, rot = shape
    q, out = _host_case(shape, dtype, fp8, 1e-6)
    assert not q[0, 0, 0].any()  # the all-zero head: zeros, no NaN
    if not fp8:
        assert not out["k"].t[0, 5, 0].any()
    # eps is seen: at 0.5 the outputs change, and still equal the composition's
    q2, _ = _host_case(shape, dtype, fp8, 0.5)
    assert not torch.equal(_qbits(q), _qbits(q2))


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_strided_qkv_rows(fp8):
    _host_case((4, 2, 128, 64), torch.bfloat16, fp8, 1e-6, strided=True)


def test_swapped_gammas_are_seen():
    """the yardstick's own sensitivity: the fused launch with q_gamma and k_gamma exchanged is NOT the composition"""
    H, Hkv, Dh, rot = 4, 2, 128, 128
    dtype = torch.bfloat16
    qkv = _tokens(6, H, Hkv, Dh, dtype, 11).view(2, 3, -1)
    qg, kg = _gammas(Dh, dtype, 12)
    fr = _angles(3, 2, rot, seed=13)
    a, b = _outputs((3, 16, Hkv, Dh), dtype, False), _outputs((3, 16, Hkv, Dh), dtype, False)
    q1 = ops.rope_kv_store_natural(qkv, fr, a["k"].t, a["v"].t, 5, H, Hkv, q_norm=qg, k_norm=kg)
    q2 = ops.rope_kv_store_natural(qkv, fr, b["k"].t, b["v"].t, 5, H, Hkv, q_norm=kg, k_norm=qg)
    torch.cuda.synchronize()
    assert not torch.equal(_qbits(q1), _qbits(q2)) and not torch.equal(a["k"].raw, b["k"].raw) and torch.equal(a["v"].raw, b["v"].raw)


def _untouched(o, outer):
    """cache rows (or pages) `outer` of every cache and scale tensor still hold their first bytes"""
    for name in o:
        if name != "q":
            assert torch.equal(o[name].t[outer].contiguous().view(torch.uint8), o[name].initial_t()[outer].contiguous().view(torch.uint8)), name


# ---- device positions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_device_positions(shape, dtype, fp8):
    H, Hkv, Dh, rot = shape
    B, S, lmax, P, eps = 3, 3, 16, 32, 1e-6
    lens = torch.tensor([4, -1, 14], dtype=torch.int32, device=DEV)  # the second is a finished slot, the third overflows lmax: both inactive
    qkv = _tokens(B * S, H, Hkv, Dh, dtype, 21).view(B, S, -1)
    qg, kg = _gammas(Dh, dtype, 22)
    table = _angles(P, rot, seed=23)
    composed = _compose(qkv, H, Hkv, Dh, qg, kg, eps)
    a, b = _outputs((B, lmax, Hkv, Dh), dtype, fp8), _outputs((B, lmax, Hkv, Dh), dtype, fp8)
    q_fused = ops.rope_kv_store_natural_pos(qkv, table, a["k"].t, a["v"].t, lens, H, Hkv, **_scales(a), q_norm=qg, k_norm=kg, norm_eps=eps)
    q_want = ops.rope_kv_store_natural_pos(composed, table, b["k"].t, b["v"].t, lens, H, Hkv, **_scales(b))
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q_fused), _qbits(q_want))
    _same(a, b)
    _no_nan(q_fused)
    # inactive sequences: zero q rows, and not a byte of their cache rows (or scales) written
    assert not q_fused[1:].any() and q_fused[0].any()
    _untouched(a, [1, 2])


# ---- paged -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_paged_chunk_across_a_page_edge(shape, dtype, fp8):
    H, Hkv, Dh, rot = shape
    B, S, page, pps, pages, P, eps = 2, 5, 64, 2, 6, 128, 1e-6
    lens = torch.tensor([62, 3], dtype=torch.int32, device=DEV)  # tokens 62 .. 66 of the first sequence cross into its second page
    bt = torch.tensor([[4, 1], [0, 5]], dtype=torch.int32, device=DEV)  # shuffled; pages 2 and 3 are nobody's
    qkv = _tokens(B * S, H, Hkv, Dh, dtype, 31).view(B, S, -1)
    qg, kg = _gammas(Dh, dtype, 32)
    table = _angles(P, rot, seed=33)
    composed = _compose(qkv, H, Hkv, Dh, qg, kg, eps)
    a, b = _outputs((pages, page, Hkv, Dh), dtype, fp8), _outputs((pages, page, Hkv, Dh), dtype, fp8)
    q_fused = ops.rope_kv_store_paged_qknorm(qkv, table, a["k"].t, a["v"].t, bt, lens, H, Hkv, **_scales(a), q_norm=qg, k_norm=kg, norm_eps=eps)
    q_want = ops.rope_kv_store_paged(composed, table, b["k"].t, b["v"].t, bt, lens, H, Hkv, **_scales(b))
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q_fused), _qbits(q_want))
    _same(a, b)
    _no_nan(q_fused)
    _untouched(a, [2, 3, 5])  # unnamed pages, and the second sequence's second page (it holds 8 tokens)
    kinit = a["k"].initial_t()
    assert not torch.equal(a["k"].t[4, 62:], kinit[4, 62:]) and not torch.equal(a["k"].t[1, :3], kinit[1, :3])  # both sides of the edge


# ---- packed steps, dense and paged ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_packed_step(shape, dtype, fp8, paged):
    H, Hkv, Dh, rot = shape
    rows, P, eps, msq = 12, 128, 1e-6, 5
    cu = torch.tensor([0, 1, 1, 6, 9], dtype=torch.int32, device=DEV)  # counts 1, 0, 5, 3; rows 9 .. 11 are padding
    # (at Dh 64 a token is 8 lanes: 9 tokens leave the second wave partly filled)
    qkv = _tokens(rows, H, Hkv, Dh, dtype, 41)
    qg, kg = _gammas(Dh, dtype, 42)
    table = _angles(P, rot, seed=43)
    composed = _compose(qkv, H, Hkv, Dh, qg, kg, eps)
    if paged:
        lens = torch.tensor([62, 3, 60, 9], dtype=torch.int32, device=DEV)  # the third sequence's 5 tokens cross a page edge
        bt = torch.tensor([[7, 2], [9, 0], [3, 8], [5, 1]], dtype=torch.int32, device=DEV)  # pages 4 and 6 are nobody's
        shape4, kw = (10, 64, Hkv, Dh), dict(block_table=bt)
    else:
        lens = torch.tensor([7, 3, 2, 9], dtype=torch.int32, device=DEV)
        shape4, kw = (4, 16, Hkv, Dh), {}
    a, b = _outputs(shape4, dtype, fp8, (rows, H, Dh)), _outputs(shape4, dtype, fp8, (rows, H, Dh))
    q_fused = ops.rope_kv_store_varq(qkv, table, a["k"].t, a["v"].t, cu, msq, lens, H, Hkv, **kw, **_scales(a), q_out=a["q"].t, q_norm=qg,
                                     k_norm=kg, norm_eps=eps)
    ops.rope_kv_store_varq(composed, table, b["k"].t, b["v"].t, cu, msq, lens, H, Hkv, **kw, **_scales(b), q_out=b["q"].t)
    torch.cuda.synchronize()
    assert q_fused.data_ptr() == a["q"].t.data_ptr()
    _same(a, b)
    qinit = a["q"].initial_t()
    assert torch.equal(_qbits(a["q"].t[9:]), _qbits(qinit[9:])) and not torch.equal(_qbits(a["q"].t[:9]), _qbits(qinit[:9]))  # the padding rows keep their bytes
    _no_nan(a["q"].t[:9])
    if paged:
        _untouched(a, [0, 1, 2, 4, 6, 9])  # every page but 7, 3, 8 and 5 (worked out below)
    else:
        _untouched(a, [1])  # the sequence that brings nothing


def test_packed_paged_page_bookkeeping_of_the_case_above():
    """which pages the paged packed case may touch, worked out on the host: sequence b writes positions lens[b] .. lens[b] + Sq_b - 1"""
    lens, counts, bt = [62, 3, 60, 9], [1, 0, 5, 3], [[7, 2], [9, 0], [3, 8], [5, 1]]
    touched = {bt[b][p // 64] for b in range(4) for p in range(lens[b], lens[b] + counts[b])}
    assert touched == {7, 3, 8, 5}


# ---- graph capture of the device-position form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_graph_replay_follows_cache_seqlens(fp8):
    H, Hkv, Dh, rot = 4, 2, 128, 64
    dtype, B, S, lmax, P, eps = torch.bfloat16, 3, 2, 16, 32, 1e-6
    qkv = _tokens(B * S, H, Hkv, Dh, dtype, 51).view(B, S, -1)
    qg, kg = (g.float() for g in _gammas(Dh, dtype, 52))  # float32 already: the wrapper converts nothing inside the capture
    table = _angles(P, rot, seed=53)
    lens = torch.tensor([0, 0, 0], dtype=torch.int32, device=DEV)
    a = _outputs((B, lmax, Hkv, Dh), dtype, fp8)
    call = lambda o, l: ops.rope_kv_store_natural_pos(qkv, table, o["k"].t, o["v"].t, l, H, Hkv, **_scales(o), q_norm=qg, k_norm=kg, norm_eps=eps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(a, lens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q_graph = call(a, lens)
    for new in ([4, -1, 9], [13, 2, 14]):
        for o in a.values():
            o.raw.copy_(o.initial)
        lens.copy_(torch.tensor(new, dtype=torch.int32, device=DEV))  # in place: the graph reads the same address
        graph.replay()
        b = _outputs((B, lmax, Hkv, Dh), dtype, fp8)
        q_eager = call(b, torch.tensor(new, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(_qbits(q_graph), _qbits(q_eager))
        _same(a, b)


# ---- the torch extension's bindings: the same launch as the ops wrappers ---------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["T", "fp8"])
def test_engine_bindings_agree_with_ops(fp8):
    E = _engine()
    H, Hkv, Dh, rot = 4, 2, 128, 64
    dtype, eps, sfx = torch.float16, 1e-5, "_fp8" if fp8 else ""
    qg, kg = (g.float() for g in _gammas(Dh, dtype, 62))
    sc = lambda o: (o["ks"].t, o["vs"].t) if fp8 else ()
    norm = dict(q_norm=qg, k_norm=kg, norm_eps=eps)
    # host position
    qkv, fr = _tokens(6, H, Hkv, Dh, dtype, 61).view(2, 3, -1), _angles(3, 2, rot, seed=63)
    a, b = _outputs((2, 16, Hkv, Dh), dtype, fp8), _outputs((2, 16, Hkv, Dh), dtype, fp8)
    q1 = getattr(E, "rope_kv_store_natural" + sfx + "_qknorm")(qkv, fr, a["k"].t, a["v"].t, *sc(a), 5, H, Hkv, qg, kg, eps)
    q2 = (ops.rope_kv_store_natural_fp8_qknorm if fp8 else ops.rope_kv_store_natural)(qkv, fr, b["k"].t, b["v"].t, *sc(b), 5, H, Hkv, **norm)
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q1), _qbits(q2))
    _same(a, b)
    # device positions, dense and paged
    table, lens = _angles(128, rot, seed=64), torch.tensor([4, 9], dtype=torch.int32, device=DEV)
    a, b = _outputs((2, 64, Hkv, Dh), dtype, fp8), _outputs((2, 64, Hkv, Dh), dtype, fp8)
    q1 = getattr(E, "rope_kv_store_natural_pos" + sfx + "_qknorm")(qkv, table, a["k"].t, a["v"].t, *sc(a), lens, H, Hkv, qg, kg, eps)
    q2 = ops.rope_kv_store_natural_pos(qkv, table, b["k"].t, b["v"].t, lens, H, Hkv, **_scales(b), **norm)
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q1), _qbits(q2))
    _same(a, b)
    bt = torch.tensor([[1], [0]], dtype=torch.int32, device=DEV)
    a, b = _outputs((2, 64, Hkv, Dh), dtype, fp8), _outputs((2, 64, Hkv, Dh), dtype, fp8)
    q1 = getattr(E, "rope_kv_store_paged_pos" + sfx + "_qknorm")(qkv, table, a["k"].t, a["v"].t, *sc(a), bt, lens, H, Hkv, qg, kg, eps)
    q2 = ops.rope_kv_store_paged_qknorm(qkv, table, b["k"].t, b["v"].t, bt, lens, H, Hkv, **_scales(b), **norm)
    torch.cuda.synchronize()
    assert torch.equal(_qbits(q1), _qbits(q2))
    _same(a, b)
    # packed, dense and paged
    cu, packed = torch.tensor([0, 2, 5], dtype=torch.int32, device=DEV), qkv.view(6, -1)
    for table_arg, kw in (((), {}), ((bt,), dict(block_table=bt))):
        a, b = _outputs((2, 64, Hkv, Dh), dtype, fp8, (6, H, Dh)), _outputs((2, 64, Hkv, Dh), dtype, fp8, (6, H, Dh))
        name = "rope_kv_store_" + ("paged" if table_arg else "natural") + "_varq" + sfx + "_qknorm"
        getattr(E, name)(packed, table, a["k"].t, a["v"].t, *sc(a), *table_arg, cu, 3, lens, H, Hkv, qg, kg, eps, a["q"].t)
        ops.rope_kv_store_varq(packed, table, b["k"].t, b["v"].t, cu, 3, lens, H, Hkv, **kw, **_scales(b), q_out=b["q"].t, **norm)
        torch.cuda.synchronize()
        _same(a, b)
    for bad in (qg.to(dtype), qg[:64].contiguous()):  # float32 [Dh] only
        with pytest.raises(RuntimeError, match="q_gamma and k_gamma"):
            getattr(E, "rope_kv_store_natural" + sfx + "_qknorm")(qkv, fr, a["k"].t, a["v"].t, *sc(a), 5, H, Hkv, bad, kg, eps)


# ---- the module ----------------------------------------------------------------------------------------------------------------------
class _ComposedQkv(torch.nn.Module):
    """a qkv layer that returns the composed qkv: what the module without the norm must be fed to give the module with it"""

    def __init__(self, H, Hkv, Dh, qg, kg, eps):
        super().__init__()
        self.cfg = (H, Hkv, Dh, qg, kg, eps)

    def forward(self, x):
        return _compose(x, *self.cfg)


def _modules(H, Hkv, Dh, L, qg, kg, eps, **kw):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused

    args = SimpleNamespace(num_attention_heads=H, num_key_value_heads=Hkv, hidden_size=H * 32, head_dim=Dh, rope_theta=10000.0, rope_scaling=None)
    fused = QuantLlamaAttentionFused(args.hidden_size, H, L, torch.nn.Identity(), torch.nn.Identity(), DEV, args, max_batch_size=2,
                                     kv_layout="natural", qk_norm=(qg, kg, eps), **kw)
    plain = QuantLlamaAttentionFused(args.hidden_size, H, L, _ComposedQkv(H, Hkv, Dh, qg, kg, eps), torch.nn.Identity(), DEV, args,
                                     max_batch_size=2, kv_layout="natural", **kw)
    assert fused.head_dim == plain.head_dim == Dh and fused.q_norm_weight.device.type == "cuda"
    return fused, plain


def _module_caches_equal(m1, m2):
    for name in ("cache_k", "cache_v", "cache_k_scale", "cache_v_scale"):
        if hasattr(m1, name):
            assert torch.equal(getattr(m1, name).view(torch.uint8), getattr(m2, name).view(torch.uint8)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_packed_split_on_the_paged_fp8_pool_with_a_window(dtype):
    H, Hkv, Dh, L, page, eps = 4, 2, 128, 256, 64, 1e-6
    qg, kg = _gammas(Dh, dtype, 72)
    fused, plain = _modules(H, Hkv, Dh, L, qg, kg, eps, kv_dtype="fp8", sliding_window=48)
    table = _angles(L, Dh, seed=73) * 0.05
    bt = torch.tensor([[5, 2, 7, 0], [1, 6, 3, 4]], dtype=torch.int32, device=DEV)
    # a prompt chunk each, then a mixed step: one decode over a history longer than the window, one chunk across a page edge
    steps = [([0, 0], [0, 70, 130]), ([70, 60], [0, 1, 8])]
    for i, (pos, cu) in enumerate(steps):
        x = _tokens(cu[-1], H, Hkv, Dh, dtype, 74 + i)[None]
        lens, cu_t = torch.tensor(pos, dtype=torch.int32, device=DEV), torch.tensor(cu, dtype=torch.int32, device=DEV)
        msq = max(b - a for a, b in zip(cu, cu[1:]))
        kw = dict(split_seqlen_q=1, split_min_keys=64, block_table=bt, page_size=page)
        got = fused.forward_packed_split(x, lens, table, cu_t, msq, **kw)
        want = plain.forward_packed_split(x, lens, table, cu_t, msq, **kw)
        torch.cuda.synchronize()
        assert got.shape == (1, cu[-1], H * Dh) and torch.equal(_qbits(got), _qbits(want)), i
        _no_nan(got)
        _module_caches_equal(fused, plain)
    assert fused.cache_k.view(torch.uint8).any()


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["T", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_forward_with_an_int_start_pos(dtype, kv_dtype):
    H, Hkv, Dh, L, eps = 4, 2, 64, 64, 1e-6
    qg, kg = _gammas(Dh, dtype, 82)
    fused, plain = _modules(H, Hkv, Dh, L, qg, kg, eps, kv_dtype=kv_dtype)
    pos = 0
    for i, S in enumerate((9, 1, 1)):
        x = _tokens(2 * S, H, Hkv, Dh, dtype, 84 + i).view(2, S, -1)
        fr = _angles(S, 2, Dh, seed=90 + i) * 0.05
        got, want = fused(x, pos, fr), plain(x, pos, fr)
        torch.cuda.synchronize()
        assert got.shape == (2, S, H * Dh) and torch.equal(_qbits(got), _qbits(want)), i
        _no_nan(got)
        _module_caches_equal(fused, plain)
        pos += S


# ---- a float32 gamma that no T holds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_float32_gamma_against_the_float64_oracle(dtype):
    """gamma = 1 + w (Gemma-3) and an angle table of zeros, so that the rotation is the identity up to the sign of zero: q_out and the T
    cache against round_T of the float64 evaluation.  Every element within 1 ulp of T; at most 2 % of them different (the error before
    the rounding -- the float32 sum, rsqrtf, two multiplies -- is far below 2^-19 relative, so a result differs only where the exact
    value lies that close to a rounding tie: about 2^-10 of the elements in bf16, 2^-7 in fp16).  tests/test_qknorm_host.py holds
    torch's own float32 evaluation of these inputs to the same bound first."""
    c = Q.ULP_CASE
    B, S, H, Hkv, Dh, eps = c["B"], c["S"], c["H"], c["Hkv"], c["Dh"], c["eps"]
    qkv, qg, kg = Q.ulp_case(dtype)
    want_q, want_k = Q.ulp_case_want(qkv, qg, kg)
    fr = torch.zeros(S, B, Dh, device=DEV)
    kc, vc = (torch.zeros(B, 16, Hkv, Dh, dtype=dtype, device=DEV) for _ in range(2))
    q = ops.rope_kv_store_natural(qkv.to(DEV), fr, kc, vc, 3, H, Hkv, q_norm=qg.to(DEV), k_norm=kg.to(DEV), norm_eps=eps)
    torch.cuda.synchronize()
    dq, dk = Q.ulp_diff(q.cpu(), want_q), Q.ulp_diff(kc[:, 3:3 + S].cpu(), want_k)
    d = torch.cat([dq.flatten(), dk.flatten()])
    share = (d != 0).float().mean().item()
    print(f"{dtype}: {d.numel()} elements, max ulp {int(d.max())}, share different {share:.5f}")
    assert int(d.max()) <= 1
    assert share <= Q.ULP_SHARE_CAP
    assert torch.equal(vc[:, 3:3 + S].cpu().view(torch.int16), qkv[..., (H + Hkv) * Dh:].reshape(B, S, Hkv, Dh).contiguous().view(torch.int16))
