"""Sliding-window attention on packed steps, without a GPU: the exports at every layer, the window plan and its workspace, the refusals of the
four C entries, of ops.attn_varq_window and of the module before any work, PageTable.release_before, and the step of tests/attn_window_cases.py:
its routes against the hand-written table, and every oracle mutant seen by at least one element of the step (`rule-sk` by a route)."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from llm_awq_amd.paged_kv import PagePoolExhausted, PageTable
from tests import attn_prefill_oracle as P
from tests import attn_window_cases as W
from tests import attn_window_oracle as O

AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
ENTRIES = ("awq_attn_varq_window", "awq_attn_varq_window_kv8", "awq_attn_paged_varq_window", "awq_attn_paged_varq_window_kv8")
MIXED = ("awq_attn_varq", "awq_attn_varq_kv8", "awq_attn_paged_varq", "awq_attn_paged_varq_kv8")
I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------------
def test_library_header_engine_and_ops_export_the_window():
    L = ctypes.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    for name in ENTRIES + ("awq_attn_varq_window_plan",):
        assert hasattr(L, name) and name in _capi.SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert hasattr(L, "awq_attn_varq_window_workspace_bytes") and re.search(r"\bsize_t awq_attn_varq_window_workspace_bytes\(", header)
    assert _capi.lib().awq_abi_version() == 1      # symbols were added, none changed
    S_ = _capi.SIGNATURES
    for new, old in zip(ENTRIES, MIXED):           # the mixed entry's arguments with window_left behind split_min_keys
        assert list(S_[new][1]) == list(S_[old][1])[:-3] + [I, VP, SZ, VP], new
    assert S_["awq_attn_varq_window_plan"][1] == [I] * 7 + [ctypes.POINTER(I)] * 2
    assert S_["awq_attn_varq_window_workspace_bytes"] == (SZ, [I] * 7)
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    tail = ["cu_seqlens_q", "max_seqlen_q", "seqlens_k", "max_seqlen_k", "split_seqlen_q", "split_min_keys", "window_left", "lens_before_step",
            "softmax_scale", "causal", "out"]
    assert params(eng.attn_varq_window) == ["q", "k_cache", "v_cache"] + tail
    assert params(eng.attn_varq_window_kv8) == ["q", "k_cache", "v_cache", "k_scale", "v_scale"] + tail
    assert params(eng.attn_paged_varq_window) == ["q", "k_pool", "v_pool", "block_table"] + tail
    assert params(eng.attn_paged_varq_window_kv8) == ["q", "k_pool", "v_pool", "k_scale", "v_scale", "block_table"] + tail
    assert params(eng.attn_varq_window_plan) == ["batch", "nheads", "nheads_kv", "head_dim", "split_seqlen_q", "max_seqlen_k", "window_left"]
    # functions of their own: ops.attn_varq and make_quant_attn keep their parameter lists
    base, win = list(inspect.signature(ops.attn_varq).parameters), list(inspect.signature(ops.attn_varq_window).parameters)
    assert "window_left" not in base and win == base[:7] + ["window_left"] + base[7:]
    assert inspect.signature(ops.attn_varq_window).parameters["window_left"].default is inspect.Parameter.empty
    assert ops.attn_varq_window_plan(4, 32, 8, 128, 1, 32768, 4095) == tuple(eng.attn_varq_window_plan(4, 32, 8, 128, 1, 32768, 4095))
    from llm_awq_amd import fused_attn

    assert inspect.signature(fused_attn.QuantLlamaAttentionFused.__init__).parameters["sliding_window"].default is None
    assert "sliding_window" not in inspect.signature(fused_attn.make_quant_attn).parameters
    assert list(inspect.signature(fused_attn.make_quant_attn_window).parameters) == ["model", "dev", "sliding_window", "max_batch_size", "kv_layout",
                                                                                      "kv_dtype"]


# ------------------------------------------------------------------------------------------------------------------------
# the plan and the workspace
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def force_chunk():
    had = os.environ.get("AWQ_TUNING")
    yield lambda c: _capi.tune(attn_splitkv_chunk=c)
    _capi.tune(attn_splitkv_chunk=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def test_window_plan_is_the_kvcache_plan_of_the_anchored_bound(force_chunk):
    L = _capi.lib()
    shapes = [(B, Hh, Hkv, Dh, q, bound, left) for B in (1, 10) for (Hh, Hkv) in ((8, 2), (32, 8)) for Dh in (64, 128) for q in (0, 1, 8)
              for bound in (1, 512, 4096, 32768, 131072) for left in (0, 1, 63, 100, 4095, 32767, 2 ** 31 - 1)]
    for forced in (0, 64, 256):
        force_chunk(forced)
        for B, Hh, Hkv, Dh, q, bound, left in shapes:
            covered = min(bound, left + q + 63)
            splits, chunk = ops.attn_varq_window_plan(B, Hh, Hkv, Dh, q, bound, left)
            assert (splits, chunk) == ops.attn_kvcache_plan(B, Hh, Hkv, Dh, max(q, 1), covered), (forced, B, Hh, Hkv, Dh, q, bound, left)
            assert splits * chunk >= covered and chunk % 64 == 0 and (not forced or chunk == forced)
            assert L.awq_attn_varq_window_workspace_bytes(B, Hh, Hkv, Dh, q, bound, left) == B * Hh * q * splits * (Dh + 2) * 4
            if left >= bound - 1:   # no window: the plan of the mixed step
                assert (splits, chunk) == ops.attn_varq_split_plan(B, Hh, Hkv, Dh, q, bound)
    force_chunk(64)
    # the step of the GPU tests: an anchored walk covers at most left + 8 + 63 keys
    assert [ops.attn_varq_window_plan(10, 8, 2, 128, 8, 512, left) for left in W.LEFTS] == [(2, 64), (2, 64), (3, 64), (3, 64), (3, 64), (5, 64), (8, 64)]
    force_chunk(0)
    assert ops.attn_varq_window_plan(32, 32, 8, 128, 1, 32768, 4095) == ops.attn_kvcache_plan(32, 32, 8, 128, 1, 4159)   # Llama-3-8B, left 4095
    s, c = ctypes.c_int(), ctypes.c_int()
    assert L.awq_attn_varq_window_plan(1, 8, 2, 128, 1, 512, 7, None, ctypes.byref(c)) == AWQ_ERR_NULL
    assert L.awq_attn_varq_window_plan(1, 8, 2, 128, 1, 512, 7, ctypes.byref(s), None) == AWQ_ERR_NULL
    refused = [(1, 8, 2, 128, 1, 512, -1), (1, 8, 2, 128, 1, 512, -2 ** 31), (1, 8, 2, 128, 33, 512, 7), (1, 8, 2, 72, 1, 512, 7),
               (1, 8, 2, 128, -1, 512, 7), (0, 8, 2, 128, 1, 512, 7), (65536, 8, 2, 128, 1, 512, 7), (1, 8, 3, 128, 1, 512, 7), (1, 8, 2, 128, 1, 0, 7)]
    for bad in refused:
        assert L.awq_attn_varq_window_plan(*bad, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE, bad
        assert L.awq_attn_varq_window_workspace_bytes(*bad) == 0, bad
        with pytest.raises(RuntimeError):
            ops.attn_varq_window_plan(*bad)
    assert L.awq_attn_varq_window_plan(1, 8, 2, 128, 32, 512, 0, ctypes.byref(s), ctypes.byref(c)) == 0


# ------------------------------------------------------------------------------------------------------------------------
# argument validation of the four entries: every call here is refused, no launch
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


OK = dict(B=3, maxq=512, total=700, before=1, bound=4096, lmax=4100, pages=40, ps=256, pps=16, trs=20, H=8, Hkv=2, Dh=128, qrs=1024,
          kbs=4100 * 256, krs=256, vbs=4100 * 256, vrs=256, ksbs=4100 * 2, ksrs=2, vsbs=4100 * 2, vsrs=2, scale=0.1, causal=1, dtype=0,
          sq=1, floor=2048, left=1023, wsb=1 << 40)


def _call(p, paged, kv8, **kw):
    a = dict(OK, q=p, k=p, v=p, ks=p, vs=p, out=p, bt=p, cu=p, lens=p, ws=p)
    if paged:
        a.update(kbs=256 * 256, vbs=256 * 256, ksbs=512, vsbs=512)
    a.update(kw)
    step = (a["B"], a["cu"], a["maxq"], a["total"], a["lens"], a["before"], a["bound"])
    where = (a["bt"], *step, a["pages"], a["ps"], a["pps"], a["trs"]) if paged else (*step, a["lmax"])
    strides = (a["qrs"], a["kbs"], a["krs"], a["vbs"], a["vrs"]) + ((a["ksbs"], a["ksrs"], a["vsbs"], a["vsrs"]) if kv8 else ())
    fn = getattr(_capi.lib(), "awq_attn_" + ("paged_" if paged else "") + "varq_window" + ("_kv8" if kv8 else ""))
    return fn(a["q"], a["k"], a["v"], *((a["ks"], a["vs"]) if kv8 else ()), a["out"], *where, a["H"], a["Hkv"], a["Dh"], *strides, a["scale"],
              a["causal"], a["dtype"], a["sq"], a["floor"], a["left"], a["ws"], a["wsb"], None)


FORMS = [(False, False), (False, True), (True, False), (True, True)]
FORM_IDS = ["dense-T", "dense-fp8", "paged-T", "paged-fp8"]


@pytest.mark.parametrize("paged,kv8", FORMS, ids=FORM_IDS)
def test_entries_refuse_without_a_launch(paged, kv8):
    buf, p = _p16()
    L = _capi.lib()
    need = L.awq_attn_varq_window_workspace_bytes(3, 8, 2, 128, 1, 4096, 1023)
    assert need == 3 * 8 * 1 * ops.attn_varq_window_plan(3, 8, 2, 128, 1, 4096, 1023)[0] * 130 * 4 > 0
    assert need < L.awq_attn_varq_split_workspace_bytes(3, 8, 2, 128, 1, 4096)          # the anchored walk is the shorter one
    # the window's own terms: a negative window and causal == 0, refused before the alignment of the lengths and the workspace are looked at
    for bad in (dict(left=-1), dict(left=-2 ** 31), dict(causal=0), dict(causal=0, left=0), dict(causal=0, left=-1)):
        assert _call(p, paged, kv8, **bad) == AWQ_ERR_SHAPE, bad
        assert _call(p, paged, kv8, lens=p + 2, ws=None, **bad) == AWQ_ERR_SHAPE, bad
    # the mixed entries' terms stay
    for bad in (dict(sq=-1), dict(floor=0), dict(sq=33), dict(maxq=0), dict(total=0), dict(B=0), dict(B=65536), dict(Dh=96), dict(H=6, Hkv=4),
                dict(qrs=512), dict(krs=128), dict(bound=0), dict(bound=4097) if paged else dict(bound=4101)):
        assert _call(p, paged, kv8, **bad) == AWQ_ERR_SHAPE, bad
    # what passes the shape phase reaches the alignment phase and, behind it, the window's workspace
    for ok in (dict(left=0), dict(left=1), dict(left=4095), dict(left=2 ** 31 - 1), dict(sq=0), dict(sq=32, left=5)):
        assert _call(p, paged, kv8, cu=p + 2, **ok) == AWQ_ERR_ALIGN, ok
        assert _call(p, paged, kv8, lens=p + 2, **ok) == AWQ_ERR_ALIGN, ok
        if ok.get("sq", 1) > 0:
            assert _call(p, paged, kv8, ws=None, **ok) == AWQ_ERR_WORKSPACE, ok
            assert _call(p, paged, kv8, wsb=0, **ok) == AWQ_ERR_WORKSPACE, ok
    assert _call(p, paged, kv8, wsb=need - 1) == AWQ_ERR_WORKSPACE        # one byte short of the WINDOW's plan
    assert _call(p, paged, kv8, wsb=need, ws=p + 4) == AWQ_ERR_ALIGN      # enough bytes: the workspace's own alignment is the last check
    assert _call(p, paged, kv8, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "cu", "lens") + (("ks", "vs") if kv8 else ()) + (("bt",) if paged else ()):
        assert _call(p, paged, kv8, **{name: None}) == AWQ_ERR_NULL, name
    # the order of the phases: null before dtype before shape (the window's terms in it) before alignment before the workspace
    assert _call(p, paged, kv8, cu=None, dtype=2, left=-1) == AWQ_ERR_NULL and _call(p, paged, kv8, dtype=2, left=-1, ws=None) == AWQ_ERR_DTYPE
    assert _call(p, paged, kv8, left=-1, cu=p + 2, ws=None) == AWQ_ERR_SHAPE and _call(p, paged, kv8, cu=p + 2, ws=None) == AWQ_ERR_ALIGN


def test_make_quant_attn_window_passes_the_window_through(monkeypatch):
    from llm_awq_amd import fused_attn

    seen = []

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = self.k_proj = self.v_proj = self.o_proj = torch.nn.Identity()
            self.args = SimpleNamespace(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, rope_theta=10000.0, sliding_window=77)
            self.kv_max_seq_len = 128
    monkeypatch.setattr(fused_attn, "fuse_qkv", lambda q, k, v: torch.nn.Identity())
    real = fused_attn.QuantLlamaAttentionFused

    def spy(*a, **kw):
        seen.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(fused_attn, "QuantLlamaAttentionFused", spy)
    monkeypatch.setattr(fused_attn, "isinstance", lambda o, c: False, raising=False)
    model = torch.nn.Sequential(Attn())
    out = fused_attn.make_quant_attn_window(model, "cpu", 33, max_batch_size=2)
    assert out[0].sliding_window == 33 and seen[-1]["sliding_window"] == 33 and seen[-1]["kv_layout"] == "natural"
    out = fused_attn.make_quant_attn(torch.nn.Sequential(Attn()), "cpu", kv_layout="natural")      # the config's 77 is never read
    assert out[0].sliding_window is None and seen[-1]["sliding_window"] is None
    with pytest.raises(ValueError, match="sliding_window"):
        fused_attn.make_quant_attn_window(torch.nn.Sequential(Attn()), "cpu", None)


def test_ops_attn_varq_window_refuses_a_bad_window_before_any_work():
    q = torch.zeros(40, 8, 128, dtype=torch.float16)
    kc = torch.zeros(2, 256, 2, 128, dtype=torch.float16)
    pool = torch.zeros(4, 64, 2, 128, dtype=torch.float16)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    lens = torch.zeros(2, dtype=torch.int32)
    for extra in (dict(), dict(block_table=bt)):
        k = pool if extra else kc
        with pytest.raises(ValueError, match="window_left -1 must not be negative"):
            ops.attn_varq_window(q, k, k, cu, 30, lens, 256, -1, **extra)
        with pytest.raises(ValueError, match="window_left.*causal"):
            ops.attn_varq_window(q, k, k, cu, 30, lens, 256, 16, causal=False, **extra)
        with pytest.raises(RuntimeError, match="GPU"):          # a good window gets as far as the GPU check, like a call without one
            ops.attn_varq_window(q, k, k, cu, 30, lens, 256, 16, **extra)
        with pytest.raises(ValueError, match="window_left must be an int"):
            ops.attn_varq_window(q, k, k, cu, 30, lens, 256, None, **extra)


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for the engine: records the entry and the arguments of every call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a, **kw):
            self.calls.append((name, a, kw))
            x = a[0]
            if name.startswith("rope_kv_store"):
                return torch.zeros(*x.shape[:-1], 8, 64, dtype=x.dtype)
            return torch.zeros_like(x)
        return fn


def _module(monkeypatch, kv_dtype=None, kv_layout="natural", **kw):
    from llm_awq_amd import fused_attn

    spy = _Spy()
    monkeypatch.setattr(fused_attn, "load_engine", lambda: spy)
    args = SimpleNamespace(num_attention_heads=8, hidden_size=512, num_key_value_heads=2, rope_theta=10000.0, sliding_window=77)
    m = fused_attn.QuantLlamaAttentionFused(512, 8, 128, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, max_batch_size=3,
                                            kv_layout=kv_layout, kv_dtype=kv_dtype, **kw)
    return m, spy


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_module_routes_every_packed_call_to_the_windowed_entries(kv_dtype, paged, monkeypatch):
    m, spy = _module(monkeypatch, kv_dtype, sliding_window=33)
    assert m.sliding_window == 33
    table = torch.zeros(3, 2, dtype=torch.int32)
    kw = dict(block_table=table, page_size=64) if paged else {}
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    name = "attn" + ("_paged" if paged else "") + "_varq_window" + ("_kv8" if kv_dtype else "")
    i = 1 + (4 if kv_dtype else 2) + paged
    out = m.forward_packed_split(x, pos, freqs, cu, 96, split_seqlen_q=2, split_min_keys=64, **kw)
    assert out.shape == (1, 140, 512) and [c[0] for c in spy.calls][1] == name and len(spy.calls) == 2
    aa = spy.calls[1][1]
    assert len(aa) == i + 10 and aa[i] is cu and aa[i + 1] == 96 and aa[i + 2] is pos and aa[i + 3] == 128
    assert aa[i + 4:i + 8] == (2, 64, 32, True) and aa[-1] is True      # the thresholds, window_left = W - 1, lens_before_step; causal
    spy.calls.clear()
    m.forward_packed(x, pos, freqs, cu, 96, **kw)                       # forward_packed is split_seqlen_q = 0
    assert spy.calls[1][0] == name and spy.calls[1][1][i + 4:i + 7] == (0, ops.ATTN_SPLIT_MIN_KEYS, 32)
    spy.calls.clear()
    xr = torch.zeros(3, 2, 768, dtype=torch.float16)                    # forward under a tensor start_pos: the uniform cu, the packed route
    out = m(xr, pos, freqs, **kw)
    assert out.shape == (3, 2, 512) and spy.calls[1][0] == name
    aa = spy.calls[1][1]
    assert aa[0].shape == (6, 8, 64) and aa[i].tolist() == [0, 2, 4, 6] and aa[i].dtype == torch.int32 and aa[i + 1] == 2 and aa[i + 2] is pos
    assert aa[i + 4:i + 7] == (2, ops.ATTN_SPLIT_MIN_KEYS, 32)
    spy.calls.clear()
    m(torch.zeros(3, 40, 768, dtype=torch.float16), pos, freqs, **kw)   # 40 * 4 rows per KV head: beyond the split pair
    assert spy.calls[1][1][i + 4] == 0


def test_module_without_a_window_is_unchanged_and_never_reads_the_config(monkeypatch):
    m, spy = _module(monkeypatch)                                       # args.sliding_window = 77 is there and is not read
    assert m.sliding_window is None
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    cu = torch.tensor([0, 40, 41, 137], dtype=torch.int32)
    x = torch.zeros(1, 140, 768, dtype=torch.float16)
    m.forward_packed(x, pos, freqs, cu, 96)
    m.forward_packed_split(x, pos, freqs, cu, 96)
    m(torch.zeros(3, 1, 768, dtype=torch.float16), pos, freqs)
    assert [c[0] for c in spy.calls] == ["rope_kv_store_natural_varq", "attn_prefill_varq", "rope_kv_store_natural_varq", "attn_varq",
                                         "rope_kv_store_natural_pos", "attn_kvcache"]


def test_module_refuses_what_the_window_is_not_built_for_before_any_work(monkeypatch):
    pos, freqs = torch.zeros(3, dtype=torch.int32), torch.zeros(128, 64)
    x = torch.zeros(3, 4, 768, dtype=torch.float16)
    m, spy = _module(monkeypatch, sliding_window=16)
    with pytest.raises(NotImplementedError, match="sliding_window.*int start_pos"):
        m(x, 0, freqs)
    with pytest.raises(NotImplementedError, match="sliding_window.*int start_pos"):
        m(x[:, :1], 5, freqs)
    ft, spy_ft = _module(monkeypatch, kv_layout="ft", sliding_window=16)
    with pytest.raises(NotImplementedError, match="sliding_window.*FT cache"):
        ft(x, 0, freqs)
    with pytest.raises(NotImplementedError, match="sliding_window.*FT cache"):
        ft(x, pos, freqs)
    with pytest.raises(NotImplementedError, match="sliding_window.*chunk_prefilling"):
        ft(x, 4, freqs, chunk_prefilling=True)
    with pytest.raises(NotImplementedError, match="sliding_window.*FT cache"):
        ft.forward_packed(x.reshape(1, 12, 768), pos, freqs, torch.tensor([0, 4, 8, 12], dtype=torch.int32), 4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="sliding_window"):
            _module(monkeypatch, sliding_window=bad)
    assert not spy.calls and not spy_ft.calls


# ------------------------------------------------------------------------------------------------------------------------
# PageTable.release_before
# ------------------------------------------------------------------------------------------------------------------------
def test_release_before_returns_dead_head_pages_and_keeps_the_page_of_the_token():
    t = PageTable(num_pages=8, page_size=64, max_batch=2, pages_per_seq=8, device="cpu")
    ptr = t.table.data_ptr()
    first = t.reserve(0, 300)                                    # 5 pages: tokens 0 .. 319
    assert first == (0, 1, 2, 3, 4) and t.free_pages == 3
    assert t.release_before(0, 0) == 0 and t.release_before(0, 63) == 0 and t.pages(0) == first       # token 63 lives in page 0
    assert t.release_before(0, 64) == 1 and t.pages(0) == (1, 2, 3, 4) and t.free_pages == 4           # page 0 lies wholly below token 64
    assert t.table[0].tolist() == [0, 1, 2, 3, 4, 0, 0, 0]
    assert t.release_before(0, 64) == 0 and t.release_before(0, 127) == 0                              # nothing twice; page 1 holds token 127
    assert t.release_before(0, 200) == 2 and t.pages(0) == (3, 4)                                      # pages 1, 2; page 3 holds token 200
    assert t.table[0].tolist() == [0, 0, 0, 3, 4, 0, 0, 0] and t.free_pages == 6                       # holes at the head of the row
    # reserve afterwards: the row grows behind its last page, at the same logical positions, from the pages just handed back
    new = t.reserve(0, 400)
    assert len(new) == 2 and set(new) <= {0, 1, 2, 5, 6, 7} and t.table[0, 5:7].tolist() == list(new) and t.table[0, :3].tolist() == [0, 0, 0]
    assert t.pages(0) == (3, 4) + new and t.reserve(0, 100) == ()                                      # never shrinks, never refills a hole
    # the pool exhausted, then refilled by release_before
    t.reserve(1, 4 * 64)
    assert t.free_pages == 0
    with pytest.raises(PagePoolExhausted):
        t.reserve(0, 449)
    assert t.release_before(0, 5 * 64 + 1) == 2 and t.free_pages == 2                                  # pages 3 and 4 of the row
    assert len(t.reserve(0, 449)) == 1 and t.free_pages == 1
    # beyond what the slot holds: everything it holds, and no more
    assert t.release_before(1, 10 ** 9) == 4 and t.pages(1) == () and t.table[1].tolist() == [0] * 8
    assert t.release_before(0, -5) == 0
    # release returns what is left and the row goes back to 0; a fresh reserve starts at position 0 again
    left = len(t.pages(0))
    assert t.release(0) == left and t.free_pages == 8 and t.table[0].tolist() == [0] * 8 and t.pages(0) == ()
    assert len(t.reserve(0, 65)) == 2 and t.table[0, 2:].tolist() == [0] * 6
    assert t.table.data_ptr() == ptr                                                                  # in place, always
    assert "max(0, Sk_b - left) & ~63" in PageTable.release_before.__doc__


def test_the_schedulers_rule_never_releases_a_key_a_later_step_reads():
    """n_tokens = max(0, Sk - left) & ~63 after a step: every later row stands at p >= Sk, and the first tile any kernel reads for it is the
    tile of its window start max(0, p - left) >= n_tokens."""
    for left in W.LEFTS + (4095,):
        for ps in (64, 128, 256):
            for sk in (1, 63, 64, 65, 300, 4096, 4097, 10000):
                n = max(0, sk - left) & ~63
                released_keys = n // ps * ps                     # pages wholly below n
                for p in (sk, sk + 1, sk + 700):
                    assert max(0, p - left) // 64 * 64 >= released_keys


# ------------------------------------------------------------------------------------------------------------------------
# the step: the one the GPU tests run, its routes by hand, and every mutant seen
# ------------------------------------------------------------------------------------------------------------------------
_ST = {}


def _step():
    if not _ST:
        _ST["st"] = W.Step(torch.bfloat16, 64)       # the loosest bound of the four combos
    return _ST["st"]


def _truth(b, left):
    key = ("ref", b, left)
    if key not in _ST:
        st = _step()
        q, k, v = st.seq(b)
        ref, A, qk = O.attention(q, k, v, left, stats=True)
        n, h = W.STEP[b]
        _ST[key] = (ref, P.bound(ref, A, qk, st.dtype, h + n, st.Dh, st.Dh ** -0.5))
    return _ST[key]


def test_step_is_the_one_the_gpu_tests_run():
    assert (W.H, W.HKV, W.BOUND, W.CHUNK, W.SPLIT_MIN_KEYS, W.SPLIT_SEQLEN_Q, W.MAX_Q, W.PAGE_SIZES) == (8, 2, 512, 64, 128, 8, 130, (64, 128))
    assert W.LEFTS == (0, 1, 63, 64, 100, 191, 511)
    assert W.STEP == ((1, 256), (8, 292), (70, 64), (130, 170), (0, 500), (1, -1), (2, 511), (3, 509), (1, 127), (4, 2))
    st = _step()
    assert st.held == [257, 300, 134, 300, 500, 0, 0, 512, 128, 6] and st.cu[-1] == 220 and st.total_q == 220 + W.PAD_ROWS and st.needles > 100
    assert [W.active(b) for b in range(10)] == [True] * 5 + [False, False] + [True] * 3
    for b, n in enumerate(st.held):     # NaN in every cache row that holds no key
        assert not torch.isnan(st.k_cache[b, :n]).any() and torch.isnan(st.k_cache[b, n:]).all() and torch.isnan(st.v_cache[b, n:]).all()
    # what the shapes were chosen for: the decode's window start at tile offsets 0, 1, 63, before key 0 and in the second page of either size
    starts = {left: 256 - left for left in W.LEFTS}
    assert {s % 64 for s in starts.values() if s >= 0} >= {0, 1, 63} and starts[511] < 0
    assert 64 <= starts[191] < 128 and 128 <= starts[100] < 256
    # the 130-row chunk at left 100: the rows of its first 128-row q tile start in tiles 1, 2 and 3
    assert {(170 + s - 100) // 64 for s in range(128)} == {1, 2, 3}
    for ps in W.PAGE_SIZES:
        pool = W.S.Pool(st, ps)
        for b, n in enumerate(st.held):
            k, v = pool.gather(b, n)
            assert torch.equal(k.view(torch.int16), st.k_cache[b, :n].view(torch.int16))


@pytest.mark.parametrize("left", W.LEFTS)
def test_routes_are_the_ones_written_down_by_hand(left):
    assert W.routes(left) == W.TAKEN[left] == W.routes(left, before=False)
    assert W.routes(left, floor=1) == W.FORCED
    wrong = W.routes(left, mutant="rule-sk")
    assert wrong == W.RULE_SK
    if left <= 100:     # Sk_b >= 128 > keys_b: the decode over 256 keys is not "long" under a short window
        assert wrong != W.routes(left) and wrong[0] and not W.routes(left)[0]
        assert 257 >= W.SPLIT_MIN_KEYS > O.window_keys(1, 257, left)
    assert O.RULE_MUTANTS == ("rule-sk",)


def test_rule_edges():
    t = lambda sq, h, left, **kw: O.takes(sq, h, True, left, kw.get("max_q", 130), kw.get("bound", 512), kw.get("split_q", 8), kw.get("floor", 128))
    assert t(1, 300, 127) and not t(1, 300, 126)                 # keys_b = left + 1
    assert t(8, 300, 120) and not t(8, 300, 119)                 # keys_b = left + Sq_b
    assert t(1, 127, 127) and t(1, 127, 4000) and not t(1, 126, 4000)     # keys_b = Sk_b once the window reaches key 0
    assert not t(9, 300, 511) and not t(0, 500, 511) and not t(1, -1, 511) and not t(2, 511, 511) and t(3, 509, 511)
    assert t(1, 2 ** 31 - 2, 2 ** 31 - 1, bound=2 ** 31 - 1)     # formed beyond 32 bits


# the lefts at which a mutant CAN be seen: at left 511 the window hides no key of a 512-key bound, so only the faults that drop a key are seen
SEEN_AT = {"left+1": W.LEFTS[:-1], "left-1": W.LEFTS, "topleft": W.LEFTS[:-1], "tile-row": W.LEFTS[:-1], "droptile": W.LEFTS,
           "nowindow": W.LEFTS[:-1]}


@pytest.mark.parametrize("mutant", O.MUTANTS)
def test_the_step_tells_every_mutant_from_the_oracle(mutant):
    st = _step()
    assert set(SEEN_AT) == set(O.MUTANTS)
    for left in SEEN_AT[mutant]:
        seen = []
        for b in range(len(W.STEP)):
            if not W.active(b) or W.STEP[b][0] == 0:
                continue
            ref, bound = _truth(b, left)
            wrong = O.attention(*st.seq(b), left, mutant=mutant)
            if not bool(((wrong - ref).abs() <= bound).all()):       # (a NaN -- a row the mutant emptied -- is a difference)
                seen.append(b)
        assert seen, (mutant, left)
        if mutant in ("left+1", "left-1", "nowindow") and left <= 100:
            assert 0 in seen, (mutant, left, seen)                    # the decode's needles stand right at the boundary


def test_oracle_is_the_prefill_oracle_plus_the_window():
    st = _step()
    for b in (1, 2, 9):
        q, k, v = st.seq(b)
        n, h = W.STEP[b]
        full = P.attention(q, k, v, causal=True, stats=True)
        mine = O.attention(q, k, v, h + n - 1, stats=True)           # left covers everything
        for a, c in zip(full, mine):
            assert torch.equal(a, c)
    # by values, on a case small enough to state: 3 rows over 5 keys (row i stands at i + 2), zero scores, v_j = j
    q = torch.zeros(1, 3, 1, 4, dtype=torch.float64)
    k = torch.zeros(1, 5, 1, 4, dtype=torch.float64)
    v = torch.arange(5, dtype=torch.float64).view(1, 5, 1, 1).expand(1, 5, 1, 4)
    assert O.attention(q, k, v, 1)[0, :, 0, 0].tolist() == [1.5, 2.5, 3.5]
    assert O.attention(q, k, v, 0)[0, :, 0, 0].tolist() == [2.0, 3.0, 4.0]
    assert O.attention(q, k, v, 1, mutant="topleft")[0, :, 0, 0].tolist() == [1.0, 1.5, 2.5]
    # a row with p < 0 is zeros: 3 rows over 2 keys
    assert O.attention(q, k[:, :2], v[:, :2], 0)[0, :, 0, 0].tolist() == [0.0, 0.0, 1.0]
