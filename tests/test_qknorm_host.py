"""not-gpu: the per-head q/k RMSNorm fused into the rope + KV-store launches (Qwen3, Gemma-3), everything that needs no launch -- the status
codes of the ten awq_rope_kv_store_*_qknorm entries, the symbols and bindings, what the `ops` wrappers refuse, the module's construction
(head_dim from the config, qk_norm on the FT cache, make_quant_attn_qknorm on a stub model), and the condition the GPU test's ulp bound
relies on, asserted on the oracle alone."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import qknorm_oracle as Q

OK, SHAPE, ALIGN, NULL = 0, -4, -5, -6
FORMS = ("natural", "natural_pos", "paged_pos", "natural_varq", "paged_varq")
ENTRIES = [f + fp8 for f in FORMS for fp8 in ("", "_fp8")]


def _args(entry, p, **over):
    """The argument list of awq_rope_kv_store_<entry>_qknorm with every pointer = p (host memory, 16-byte aligned: no check reads it) and
    a shape every check accepts; `over` replaces named arguments."""
    fp8, form = entry.endswith("_fp8"), entry[:-4] if entry.endswith("_fp8") else entry
    H, Hkv, Dh = 4, 2, 128
    row = Hkv * Dh
    a = dict(qkv=p, freqs=p, q_gamma=p, k_gamma=p, norm_eps=1e-6, q_out=p, k=p, v=p)
    if fp8:
        a.update(k_scale=p, v_scale=p)
    paged, packed = form.startswith("paged"), form.endswith("varq")
    if paged:
        a.update(block_table=p)
    if form != "natural":
        a.update(cache_seqlens=p)
    a.update(batch=2)
    if not paged:
        a.update(cache_batch=2)
    if packed:
        a.update(cu_seqlens_q=p, max_seqlen_q=3, total_q=6)
    else:
        a.update(seqlen=3)
    a.update(nheads=H, nheads_kv=Hkv, head_dim=Dh, rot_dim=Dh)
    if not paged:
        a.update(lmax=16)
    if form == "natural":
        a.update(start_pos=5)
    else:
        a.update(table_rows=32)
    if paged:
        a.update(num_pages=4, page_size=64, pages_per_seq=2, table_row_stride=2, k_page_stride=64 * row, k_row_stride=row,
                 v_page_stride=64 * row, v_row_stride=row)
        if fp8:
            a.update(ks_page_stride=64 * Hkv, ks_row_stride=Hkv, vs_page_stride=64 * Hkv, vs_row_stride=Hkv)
    if not packed:
        a.update(qkv_batch_stride=3 * (H + 2 * Hkv) * Dh)
    a.update(qkv_row_stride=(H + 2 * Hkv) * Dh, dtype=_capi.AWQ_BF16, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return list(a.values())


@pytest.fixture(scope="module")
def host_ptr():
    buf = (ctypes.c_char * 256)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.mark.parametrize("entry", ENTRIES)
def test_status_codes_of_the_qknorm_entries_without_a_launch(entry, host_ptr):
    _, p = host_ptr
    fn = getattr(_capi.lib(), "awq_rope_kv_store_" + entry + "_qknorm")
    sig = _capi.SIGNATURES["awq_rope_kv_store_" + entry + "_qknorm"][1]
    assert len(_args(entry, p)) == len(sig)
    # the norm's own terms, each in its phase
    assert fn(*_args(entry, p, q_gamma=None)) == NULL
    assert fn(*_args(entry, p, k_gamma=None)) == NULL
    assert fn(*_args(entry, p, q_gamma=p + 4)) == ALIGN
    assert fn(*_args(entry, p, k_gamma=p + 8)) == ALIGN
    for eps in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert fn(*_args(entry, p, norm_eps=eps)) == SHAPE, eps
    # the phases keep their order: NULL before SHAPE before ALIGN
    assert fn(*_args(entry, p, k_gamma=None, norm_eps=-1.0, q_gamma=p + 4)) == NULL
    assert fn(*_args(entry, p, norm_eps=-1.0, q_gamma=p + 4)) == SHAPE
    # and the sibling's rules are inherited: one shape error, one NULL, one misaligned pointer
    assert fn(*_args(entry, p, head_dim=96)) == SHAPE
    assert fn(*_args(entry, p, rot_dim=24)) == SHAPE
    assert fn(*_args(entry, p, qkv=None)) == NULL
    assert fn(*_args(entry, p, q_out=p + 2)) == ALIGN
    assert fn(*_args(entry, p, dtype=7)) == -3


def test_symbols_are_exported_declared_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    header = open(llm_awq_amd.__file__.replace("llm_awq_amd/__init__.py", "include/awq_cdna4.h")).read()
    eng = llm_awq_amd.load_engine()
    for entry in ENTRIES:
        name = "awq_rope_kv_store_" + entry + "_qknorm"
        assert hasattr(L, name) and name in _capi.SIGNATURES and ("int " + name + "(") in header, name
        # the sibling's arguments with q_gamma, k_gamma, norm_eps directly after the angles
        base, mine = _capi.SIGNATURES["awq_rope_kv_store_" + entry][1], _capi.SIGNATURES[name][1]
        assert mine == base[:2] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float] + base[2:]
        assert callable(getattr(eng, "rope_kv_store_" + entry + "_qknorm")) and callable(getattr(eng, "rope_kv_store_" + entry))
        assert "q_gamma" in getattr(eng, "rope_kv_store_" + entry + "_qknorm").__doc__


def test_ops_wrappers_take_the_norm_by_keyword_only_and_refuse_cpu_tensors_and_a_lone_gamma():
    # (rope_kv_store_natural_fp8 and rope_kv_store_paged keep their parameter lists: the norm is their _qknorm siblings')
    wrappers = (ops.rope_kv_store_natural, ops.rope_kv_store_natural_fp8_qknorm, ops.rope_kv_store_natural_pos, ops.rope_kv_store_paged_qknorm,
                ops.rope_kv_store_varq)
    for plain, sibling in ((ops.rope_kv_store_natural_fp8, wrappers[1]), (ops.rope_kv_store_paged, wrappers[3])):
        ps = list(inspect.signature(sibling).parameters)
        assert ps[:-3] == list(inspect.signature(plain).parameters) and ps[-3:] == ["q_norm", "k_norm", "norm_eps"]
    for fn in wrappers:
        ps = inspect.signature(fn).parameters
        for name, default in (("q_norm", None), ("k_norm", None), ("norm_eps", 1e-6)):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default == default, (fn.__name__, name)
    H, Hkv, Dh = 2, 1, 64
    qkv = torch.zeros(1, 2, (H + 2 * Hkv) * Dh, dtype=torch.bfloat16)
    fr, kc, vc = torch.zeros(2, 1, Dh), torch.zeros(1, 8, Hkv, Dh, dtype=torch.bfloat16), torch.zeros(1, 8, Hkv, Dh, dtype=torch.bfloat16)
    ks, lens, g = torch.zeros(1, 8, Hkv), torch.zeros(1, dtype=torch.int32), torch.ones(Dh)
    bt, cu = torch.zeros(1, 1, dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)
    calls = [lambda **kw: ops.rope_kv_store_natural(qkv, fr, kc, vc, 0, H, Hkv, **kw),
             lambda **kw: ops.rope_kv_store_natural_fp8_qknorm(qkv, fr, kc, vc, ks, ks, 0, H, Hkv, **kw),
             lambda **kw: ops.rope_kv_store_natural_pos(qkv, fr[:, 0], kc, vc, lens, H, Hkv, **kw),
             lambda **kw: ops.rope_kv_store_paged_qknorm(qkv, fr[:, 0], kc, vc, bt, lens, H, Hkv, **kw),
             lambda **kw: ops.rope_kv_store_varq(qkv[0], fr[:, 0], kc, vc, cu, 2, lens, H, Hkv, **kw)]
    for call in calls:
        with pytest.raises(_capi.AwqNativeError, match="GPU only"):
            call(q_norm=g, k_norm=g)
        with pytest.raises(ValueError, match="q_norm and k_norm come together"):
            call(q_norm=g)
        with pytest.raises(ValueError, match="q_norm and k_norm come together"):
            call(k_norm=g)


# ---- the module, built on the CPU (nothing is launched) --------------------------------------------------------------------------
def _cfg(**kw):
    return SimpleNamespace(**{**dict(hidden_size=1024, num_attention_heads=16, num_key_value_heads=8, rope_theta=1e6, rope_scaling=None), **kw})


def _attn(args, **kw):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused

    return QuantLlamaAttentionFused(args.hidden_size, args.num_attention_heads, 64, torch.nn.Identity(), torch.nn.Identity(), "cpu", args, **kw)


def test_head_dim_comes_from_the_config_where_it_declares_one():
    m = _attn(_cfg(head_dim=128), kv_layout="natural")  # Qwen3-0.6B: hidden 1024, 16 heads, head_dim 128
    assert m.head_dim == 128 and tuple(m.cache_k.shape) == (1, 64, 8, 128)
    assert _attn(_cfg(), kv_layout="natural").head_dim == 64 and _attn(_cfg(head_dim=None), kv_layout="natural").head_dim == 64
    assert tuple(_attn(_cfg(head_dim=128)).cache_k.shape) == (1, 8, 16, 64, 8)  # the FT cache follows it too
    with pytest.raises(ValueError, match="head dim 96"):
        _attn(_cfg(head_dim=96), kv_layout="natural")


def test_module_holds_the_norm_as_float32_buffers_and_refuses_the_ft_cache():
    w = (1.0 + 0.05 * torch.randn(128)).to(torch.bfloat16)
    m = _attn(_cfg(head_dim=128), kv_layout="natural", kv_dtype="fp8", sliding_window=32, qk_norm=(w, 2 * w, 1e-5))
    assert m.q_norm_weight.dtype == m.k_norm_weight.dtype == torch.float32 and m.qk_norm_eps == 1e-5
    assert torch.equal(m.q_norm_weight, w.float()) and torch.equal(m.k_norm_weight, (2 * w).float())
    assert set(dict(m.named_buffers())) == {"q_norm_weight", "k_norm_weight"}  # so .to(dev) moves them
    plain = _attn(_cfg(head_dim=128), kv_layout="natural")
    assert plain.qk_norm_eps is None and not dict(plain.named_buffers())
    with pytest.raises(NotImplementedError, match="qk_norm is not implemented on the FT cache"):
        _attn(_cfg(head_dim=128), qk_norm=(w, w, 1e-6))
    with pytest.raises(ValueError, match=r"\[head_dim\] = \[128\]"):
        _attn(_cfg(head_dim=128), kv_layout="natural", qk_norm=(w[:64], w, 1e-6))
    with pytest.raises(ValueError, match="eps"):
        _attn(_cfg(head_dim=128), kv_layout="natural", qk_norm=(w, w, -1.0))


class _Norm(torch.nn.Module):
    def __init__(self, w, **eps):
        super().__init__()
        self.weight = torch.nn.Parameter(w)
        for k, v in eps.items():
            setattr(self, k, v)


class _StubAttention(torch.nn.Module):
    def __init__(self, qw, kw, eps_name="variance_epsilon"):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = (torch.nn.Identity() for _ in range(4))
        self.args, self.kv_max_seq_len = _cfg(head_dim=128), 64
        self.q_norm, self.k_norm = _Norm(qw, **{eps_name: 1e-5}), _Norm(kw, **{eps_name: 1e-5})


def _stub_model(monkeypatch, **kw):
    from llm_awq_amd import fused_attn

    monkeypatch.setattr(fused_attn, "fuse_qkv", lambda q, k, v: torch.nn.Identity())  # the projections are not under test
    qw, kw_ = (0.1 * torch.randn(128)).to(torch.bfloat16), (0.1 * torch.randn(128)).to(torch.bfloat16)
    model = torch.nn.Module()
    model.layer = torch.nn.Module()
    model.layer.self_attn = _StubAttention(qw, kw_, **kw)
    return model, qw, kw_


@pytest.mark.parametrize("eps_name", ["variance_epsilon", "eps"])
def test_make_quant_attn_qknorm_picks_up_weights_eps_and_offset(monkeypatch, eps_name):
    from llm_awq_amd.fused_attn import QuantLlamaAttentionFused, make_quant_attn_qknorm

    for offset in (0.0, 1.0):
        model, qw, kw = _stub_model(monkeypatch, eps_name=eps_name)
        make_quant_attn_qknorm(model, "cpu", kv_dtype="fp8", sliding_window=16, norm_offset=offset)
        m = model.layer.self_attn
        assert isinstance(m, QuantLlamaAttentionFused) and m.kv_layout == "natural" and m.kv_dtype == "fp8" and m.sliding_window == 16
        assert m.head_dim == 128 and m.qk_norm_eps == 1e-5
        assert torch.equal(m.q_norm_weight, offset + qw.float()) and torch.equal(m.k_norm_weight, offset + kw.float())  # (1 + w) in float32
        assert not torch.equal(m.q_norm_weight, m.k_norm_weight)
    assert list(inspect.signature(make_quant_attn_qknorm).parameters) == ["model", "dev", "max_batch_size", "kv_layout", "kv_dtype",
                                                                         "sliding_window", "norm_offset"]


def test_make_quant_attn_refuses_a_module_with_a_norm_and_names_the_new_function(monkeypatch):
    from llm_awq_amd.fused_attn import make_quant_attn, make_quant_attn_qknorm, make_quant_attn_window

    for build in (lambda m: make_quant_attn(m, "cpu", kv_layout="natural"), lambda m: make_quant_attn_window(m, "cpu", 16)):
        model, _, _ = _stub_model(monkeypatch)
        with pytest.raises(ValueError, match="make_quant_attn_qknorm"):
            build(model)
        assert isinstance(model.layer.self_attn, _StubAttention)  # nothing was replaced
    model, _, _ = _stub_model(monkeypatch)
    model.layer.self_attn.k_norm = None  # a lone norm is no Qwen3 / Gemma-3 block
    with pytest.raises(ValueError, match="both q_norm and k_norm"):
        make_quant_attn_qknorm(model, "cpu")
    with pytest.raises(ValueError, match="make_quant_attn_qknorm"):
        make_quant_attn(model, "cpu", kv_layout="natural")


# ---- the condition of the GPU test's ulp bound, on the oracle alone ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_float32_evaluation_stays_within_the_ulp_bound_of_float64(dtype):
    """tests/test_gpu_qknorm.py compares the fused launch under a float32 gamma that no T holds with round_T of the float64 evaluation:
    every element within 1 ulp of T and at most ULP_SHARE_CAP of them different.  The cap is a condition on the inputs, not a
    measurement of the kernel: torch's own float32 evaluation of the same inputs -- another order of the sum, another rsqrt -- must stay
    within it too, or the case would say nothing."""
    qkv, qg, kg = Q.ulp_case(dtype)
    c = Q.ULP_CASE
    H, Hkv, Dh = c["H"], c["Hkv"], c["Dh"]
    want_q, want_k = Q.ulp_case_want(qkv, qg, kg)
    got = Q.compose(qkv, H, Hkv, Dh, qg, kg, c["eps"])
    got_q = got[..., :H * Dh].reshape(want_q.shape)
    got_k = got[..., H * Dh:(H + Hkv) * Dh].reshape(want_k.shape)
    d = torch.cat([Q.ulp_diff(got_q, want_q).flatten(), Q.ulp_diff(got_k, want_k).flatten()])
    share = (d != 0).float().mean().item()
    print(f"{dtype}: {d.numel()} elements, max ulp {int(d.max())}, share different {share:.5f}")
    assert d.numel() == c["B"] * c["S"] * (H + Hkv) * Dh and int(d.max()) <= 1 and share <= Q.ULP_SHARE_CAP
    # the gamma matters: rounding it to T first moves far more elements than the cap allows
    lossy = Q.compose(qkv, H, Hkv, Dh, qg.to(dtype), kg.to(dtype), c["eps"])
    assert (Q.ulp_diff(lossy[..., :H * Dh].reshape(want_q.shape), want_q) != 0).float().mean().item() > 5 * Q.ULP_SHARE_CAP
    # and the ulp arithmetic: neighbours are 1 apart, the two zeros 0
    one = torch.tensor([1.0, -1.0, 0.0], dtype=dtype)
    nxt = (one.view(torch.int16) + 1).view(dtype)
    assert Q.ulp_diff(one, nxt).tolist() == [1, 1, 1] and Q.ulp_diff(torch.tensor([0.0], dtype=dtype), torch.tensor([-0.0], dtype=dtype)).item() == 0
