"""Encoder-tower attention without a GPU: the soundness of the needle inputs of tests/attn_tower_cases.py against the float64 oracle (the
list objects tests/test_gpu_attention_tower.py runs through the kernel), the C ABI's argument checks and host plan, the flash_attn
submodules the vision towers import, and the generated ISA of csrc/awq_attn_tower_cdna4.hip."""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_oracle as O
from tests import attn_tower_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL = -3, -4, -5, -6


# ------------------------------------------------------------------------------------------------------------------------
# the needle inputs are sound
# ------------------------------------------------------------------------------------------------------------------------
def _dense_oracle(case, mutant=None):
    q = case.q
    if mutant == "tail":
        q = q.clone()
        q[..., 64:] = 0
        mutant = None
    return O.attention(q, case.k, case.v, case.scale, False, mutant=mutant)


def test_case_lists_cover_the_axes_of_the_issue():
    sq = {(s["Sq"], s["Sk"]) for s in C.DENSE}
    for S in (1, 63, 64, 65, 127, 129, 200, 729):
        assert (S, S) in sq
    assert (100, 333) in sq and (333, 100) in sq
    assert all(s["Dh"] == 72 and not s["causal"] for s in C.DENSE)
    assert any(s["H"] == 4 and s["Hkv"] == 2 for s in C.DENSE) and max(s["B"] for s in C.DENSE) == 3
    assert {s.get("pair") for s in C.DENSE} >= {(63, 64), (0, 728)}
    assert {s["mode"] for s in C.DENSE} == {"scatter", "edges", "zero", "diag", "negscale", "pair"}
    assert {s["dtype"] for s in C.DENSE} == set(C.DTYPES) == {s["dtype"] for s in C.VARLEN}
    lens = {(tuple(s["lens"]), s["Dh"]) for s in C.VARLEN}
    for want in ((1, 65, 0, 200, 729), (64, 64, 64), (129,)):
        assert (want, 64) in lens and (want, 72) in lens
    assert ((1025, 1025), 64) in lens
    assert any(s.get("max_seqlen", 0) > max(s["lens"]) for s in C.VARLEN)
    assert len({s["name"] for s in C.DENSE + C.VARLEN}) == len(C.DENSE) + len(C.VARLEN)
    assert 2 * 32 * (72 // 16) / 72 ** 0.5 >= C.GAP_MIN and abs(C.gap(72) - 30.17) < 0.01


@pytest.mark.parametrize("spec", C.DENSE, ids=C.case_id)
def test_dense_oracle_alone_returns_the_targets_and_sees_faults(spec):
    case = C.dense_case(spec)
    for t in case.backing:  # the padding is NaN, the views are not
        assert torch.isnan(t).any()
    assert not (torch.isnan(case.q).any() or torch.isnan(case.k).any() or torch.isnan(case.v).any())
    out = _dense_oracle(case)
    assert float((out - case.target.double()).abs().max()) < 2.0 ** -16
    assert torch.equal(out.to(case.dtype), case.target)
    for mutant in C.MUTANTS:
        if C.mutant_applies(case, mutant):
            assert not torch.equal(_dense_oracle(case, mutant).to(case.dtype), case.target), mutant


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_tail_needle_lives_in_the_ninth_chunk(dtype):
    case = C.TailCase(dtype)
    assert not case.q[..., :64].any() and not case.k[..., :64].any() and case.scale == 1.0
    s = torch.einsum("bihd,bjhd->bhij", case.q.double(), case.k.double())
    top = s.max(-1).values
    assert (top == 256).all() and (s.masked_fill(s == 256, 0).max() <= 192)
    out = _dense_oracle(case)
    assert torch.equal(out.to(dtype), case.target)
    assert C.mutant_applies(case, "tail") and not torch.equal(_dense_oracle(case, "tail").to(dtype), case.target)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d)[6:])
def test_poisoned_neighbours_leave_head_one_exact(dtype):
    case = C.poisoned(dtype)
    for t in (case.q, case.k, case.v):
        assert torch.isnan(t[:, :, 0]).all() and torch.isnan(t[:, :, 2]).all() and not torch.isnan(t[:, :, 1]).any()
    out = _dense_oracle(case)
    assert torch.equal(out[:, :, 1].to(dtype), case.target[:, :, 1])
    assert torch.isnan(out[:, :, 0]).all() and torch.isnan(out[:, :, 2]).all()


@pytest.mark.parametrize("spec", C.VARLEN, ids=C.case_id)
def test_varlen_oracle_alone_returns_the_targets_and_sees_faults(spec):
    case = C.VarlenCase(spec)
    assert torch.isnan(case.qkv[case.total:]).all() and not torch.isnan(case.qkv[:case.total]).any()
    out = C.varlen_oracle(case.qkv, case.cu, case.max_seqlen)
    assert float((out - case.target.double()).abs().max()) < 2.0 ** -16
    assert torch.equal(out.to(case.dtype), case.target)
    for mutant in C.MUTANTS:
        if C.mutant_applies(case, mutant):
            bad = C.varlen_oracle(case.qkv, case.cu, case.max_seqlen, mutant=mutant)
            assert not torch.equal(bad.to(case.dtype), case.target), mutant


def test_every_fault_is_seen_by_some_case():
    seen = {m: 0 for m in C.MUTANTS}
    cases = [C.dense_case(s) for s in C.DENSE if s["Sq"] <= 200] + [C.VarlenCase(s) for s in C.VARLEN] + [C.TailCase(torch.float16)]
    for case in cases:
        for m in C.MUTANTS:
            seen[m] += C.mutant_applies(case, m)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------------------
# C ABI: argument checks, plan
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _varlen(p, **kw):
    a = dict(q=p, k=p, v=p, out=p, cu=p, nseq=2, maxs=16, total=32, H=4, Dh=72, qrs=3 * 288, krs=3 * 288, vrs=3 * 288, scale=0.1, causal=0, dtype=0)
    a.update(kw)
    return _capi.lib().awq_attn_varlen(a["q"], a["k"], a["v"], a["out"], a["cu"], a["nseq"], a["maxs"], a["total"], a["H"], a["Dh"], a["qrs"],
                                       a["krs"], a["vrs"], a["scale"], a["causal"], a["dtype"], None)


def test_library_and_engine_export_the_tower_surface():
    L = _capi.lib()
    assert hasattr(L, "awq_attn_varlen") and hasattr(L, "awq_attn_varlen_plan") and L.awq_abi_version() == 1
    doc = llm_awq_amd.load_engine().attn_varlen_qkvpacked.__doc__.splitlines()[0]
    params = [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params == ["qkv", "cu_seqlens", "max_seqlen", "softmax_scale", "causal"], doc


def test_varlen_argument_validation_returns_codes_without_launch():
    buf, p = _p16()
    for bad in (dict(Dh=128), dict(Dh=32), dict(Dh=80), dict(causal=1), dict(nseq=0), dict(maxs=0), dict(total=0), dict(H=0), dict(qrs=280),
                dict(krs=280), dict(vrs=280), dict(nseq=-1), dict(maxs=-5)):
        assert _varlen(p, **bad) == AWQ_ERR_SHAPE, bad
    assert _varlen(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out", "cu"):
        assert _varlen(p, **{name: None}) == AWQ_ERR_NULL, name
    for name in ("q", "k", "v", "out"):
        assert _varlen(p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    assert _varlen(p, cu=p + 2) == AWQ_ERR_ALIGN
    for name in ("qrs", "krs", "vrs"):
        assert _varlen(p, **{name: 3 * 288 + 4}) == AWQ_ERR_ALIGN, name
    r, n = ctypes.c_int(), ctypes.c_int()
    L = _capi.lib()
    for bad in ((0, 16, 72, 729), (1, 0, 72, 729), (1, 16, 128, 729), (1, 16, 96, 729), (1, 16, 72, 0)):
        assert L.awq_attn_varlen_plan(*bad, ctypes.byref(r), ctypes.byref(n)) == AWQ_ERR_SHAPE, bad
    assert L.awq_attn_varlen_plan(1, 16, 72, 729, None, ctypes.byref(n)) == AWQ_ERR_NULL
    assert L.awq_attn_varlen_plan(1, 16, 72, 729, ctypes.byref(r), None) == AWQ_ERR_NULL
    assert L.awq_attn_varlen_plan(1, 16, 72, 729, ctypes.byref(r), ctypes.byref(n)) == 0


def _prefill(p, **kw):
    a = dict(q=p, k=p, v=p, out=p, B=1, Sq=16, Sk=16, H=4, Hkv=2, Dh=72, qbs=16 * 288, qrs=288, kbs=16 * 144, krs=144, vbs=16 * 144, vrs=144,
             scale=0.1, causal=0, dtype=0)
    a.update(kw)
    return _capi.lib().awq_attn_prefill(a["q"], a["k"], a["v"], a["out"], a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"],
                                        a["kbs"], a["krs"], a["vbs"], a["vrs"], a["scale"], a["causal"], a["dtype"], None)


def test_prefill_entry_admits_head_dim_72_without_a_mask_only():
    buf, p = _p16()
    # the alignment check follows the shape check: a misaligned pointer is reported only once the shape has passed
    assert _prefill(p, out=p + 2) == AWQ_ERR_ALIGN
    assert _prefill(p, Sq=20, Sk=16, out=p + 2) == AWQ_ERR_ALIGN
    assert _prefill(p, causal=1) == AWQ_ERR_SHAPE and _prefill(p, causal=1, out=p + 2) == AWQ_ERR_SHAPE
    assert _prefill(p, qrs=280) == AWQ_ERR_SHAPE and _prefill(p, H=3) == AWQ_ERR_SHAPE
    assert ops.attn_prefill_plan(1, 16, 16, 72, 729, 729, False) == ops.attn_varlen_plan(1, 16, 72, 729)
    r, n = ctypes.c_int(), ctypes.c_int()
    assert _capi.lib().awq_attn_prefill_plan(1, 16, 16, 72, 729, 729, 1, ctypes.byref(r), ctypes.byref(n)) == AWQ_ERR_SHAPE


# (q_tile_rows, blocks) of the four tower shapes (DESIGN.md "Tower attention"): 64-row tiles while 128-row tiles leave fewer than two
# blocks per CU, 128 rows otherwise
TOWERS = {("siglip", 1): (16, 72, 729, 64, 192), ("siglip", 8): (16, 72, 729, 128, 768),
          ("internvit", 1): (16, 64, 1025, 64, 272), ("internvit", 8): (16, 64, 1025, 128, 1152)}


@pytest.mark.parametrize("key", sorted(TOWERS))
def test_plan_is_pinned_for_the_towers_and_covers_the_rows(key):
    H, Dh, S, rows, blocks = TOWERS[key]
    B = key[1]
    assert ops.attn_varlen_plan(B, H, Dh, S) == (rows, blocks)
    assert rows % 32 == 0 and blocks % (B * H) == 0
    tiles = blocks // (B * H)
    assert tiles * rows >= S > (tiles - 1) * rows


# ------------------------------------------------------------------------------------------------------------------------
# the flash_attn names the towers import
# ------------------------------------------------------------------------------------------------------------------------
_SHIM = r"""
import sys, importlib.util
real = importlib.util.find_spec("flash_attn") is not None  # (a machine with the CUDA package: it is left alone unless forced)
import llm_awq_amd
if not real:
    other = type(sys)("flash_attn"); sys.modules["flash_attn"] = other
    assert llm_awq_amd.install_as_flash_attn() is other and "flash_attn.bert_padding" not in sys.modules  # left alone: nothing registered
    assert "flash_attn.flash_attn_interface" not in sys.modules
m = llm_awq_amd.install_as_flash_attn(force=True)
assert sys.modules["flash_attn"] is m and m.__name__ == "llm_awq_amd.flash_attn_compat"
# the import lines of internvit.py:18-20 and fused_siglipdecoder.py:15
from flash_attn.bert_padding import pad_input, unpad_input
from flash_attn.flash_attn_interface import flash_attn_varlen_qkvpacked_func
from flash_attn import flash_attn_func
import flash_attn.flash_attn_interface, flash_attn.bert_padding
assert flash_attn.flash_attn_interface.flash_attn_func is flash_attn_func is m.flash_attn_func
assert flash_attn_varlen_qkvpacked_func is m.flash_attn_varlen_qkvpacked_func
from flash_attn.bert_padding import index_first_axis
before = dict((k, sys.modules[k]) for k in ("flash_attn", "flash_attn.flash_attn_interface", "flash_attn.bert_padding"))
assert llm_awq_amd.install_as_flash_attn() is m and all(sys.modules[k] is v for k, v in before.items())  # a second call changes nothing

import torch
torch.manual_seed(0)
B, S, D = 3, 7, 5
mask = torch.tensor([[1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0, 0]], dtype=torch.bool)
x = torch.randn(B, S, D)
xu, idx, cu, mx = unpad_input(x, mask)
assert xu.shape == (11, D) and cu.dtype == torch.int32 and cu.tolist() == [0, 3, 10, 11] and isinstance(mx, int) and mx == 7
assert torch.equal(xu, x[mask]) and torch.equal(index_first_axis(x.reshape(B * S, D), idx), xu)
back = pad_input(xu, idx, B, S)
assert back.shape == x.shape and torch.equal(back, x * mask[..., None])
xu3, _, _, _ = unpad_input(x.reshape(B, S, 1, D).expand(B, S, 3, D).contiguous(), mask.int())  # internvit.py:74 passes [B, S, 3 H D]-like trailing dims
assert xu3.shape == (11, 3, D)

qkv = torch.zeros(4, 3, 2, 64, dtype=torch.float16)
cus = torch.tensor([0, 4], dtype=torch.int32)
for kw, word in ((dict(dropout_p=0.1), "dropout_p"), (dict(causal=True), "causal"), (dict(window_size=(128, 0)), "window_size"),
                 (dict(alibi_slopes=torch.ones(2)), "alibi_slopes"), (dict(return_attn_probs=True), "return_attn_probs"), (dict(softcap=30.0), "softcap")):
    try:
        flash_attn_varlen_qkvpacked_func(qkv, cus, 4, **kw)
    except NotImplementedError as e:
        assert word in str(e), (word, str(e))
    else:
        raise AssertionError(word)
assert not torch.cuda.is_initialized()
try:  # the "off" values pass the keyword check and reach the engine, which refuses CPU tensors
    flash_attn_varlen_qkvpacked_func(qkv, cus, 4, 0.0, softmax_scale=None, causal=False, window_size=(-1, -1), alibi_slopes=None, deterministic=True,
                                     return_attn_probs=False)
except RuntimeError as e:
    assert not isinstance(e, NotImplementedError) and "GPU" in str(e), str(e)
else:
    raise AssertionError("CPU tensors were accepted")
q = torch.zeros(1, 4, 2, 72, dtype=torch.float16)
try:
    flash_attn_func(q, q, q, causal=False)
except RuntimeError as e:
    assert "GPU" in str(e), str(e)
else:
    raise AssertionError("CPU tensors were accepted")
assert not torch.cuda.is_initialized()
print("shim ok")
"""


def test_tower_imports_resolve_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", _SHIM], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------------
# generated code
# ------------------------------------------------------------------------------------------------------------------------
# every instantiation the launch code can reach: 2 dtypes x 2 head dims x {1, 2, 4} waves (q tiles of 32, 64 and 128 rows)
INSTANCES = {(dt, dh, nw): f"attn_tower_kernelINS_{tag}ELi{dh}ELi{nw}EE" for dt, tag in (("f16", "3F16"), ("bf16", "4BF16")) for dh in (64, 72)
             for nw in (1, 2, 4)}


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
               os.path.join(ROOT, "llm_awq_amd", "csrc"), "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=16",
               "-S", "--cuda-device-only", os.path.join(ROOT, "llm_awq_amd", "csrc", "awq_attn_tower_cdna4.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        text = open(out).read().split("\n")
    found = {}
    for key, frag in INSTANCES.items():
        starts = [i for i, ln in enumerate(text) if ln.startswith("_ZN3awq") and ":" in ln and frag in ln.split(":")[0]]
        assert len(starts) == 1, (key, len(starts))
        s = starts[0]
        e = next(i for i in range(s, len(text)) if text[i].strip().startswith(".size"))
        body = [ln.strip() for ln in text[s + 1:e]]
        body = [ln for ln in body if ln and not ln.startswith(";") and "ASMSTART" not in ln and "ASMEND" not in ln]
        sym = text[s].split(":")[0]
        meta = next(i for i, ln in enumerate(text) if ln.strip() == f".name:           {sym}")
        ind = len(text[meta]) - len(text[meta].lstrip())  # the keys of one kernel's metadata entry share this indentation
        top = lambda j: text[j].startswith(" " * (ind - 2) + "- .")
        lo = max(j for j in range(meta + 1) if top(j))
        hi = next((j for j in range(meta + 1, len(text)) if top(j) or not text[j].startswith(" " * (ind - 2))), len(text))
        found[key] = (body, "\n".join(text[lo:hi]))
    return found


@pytest.mark.parametrize("key", sorted(INSTANCES))
def test_generated_code_uses_the_matrix_cores_and_no_scratch(isa, key):
    body, meta = isa[key]
    dt = key[0]
    assert any(ln.startswith(f"v_mfma_f32_32x32x16_{dt}") for ln in body)
    assert not any(ln.startswith("v_mfma") and f"_{dt}" not in ln for ln in body)
    assert ".private_segment_fixed_size: 0" in meta, meta
    assert not any(ln.startswith("scratch_") for ln in body)
