"""Prefill attention without a GPU: the exports, the C ABI's argument checks and host plan, the flash_attn shim, the generated ISA of
the kernel (csrc/awq_attn_prefill_cdna4.hip), and the soundness of the needle inputs of tests/attn_prefill_cases.py against the float64
oracle (tests/attn_prefill_oracle.py) -- the list object tests/test_gpu_attention_prefill.py runs through the kernel."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_cases as C
from tests import attn_prefill_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL = -3, -4, -5, -6


def test_library_and_engine_export_the_prefill_surface():
    L = _capi.lib()
    for name in ("awq_attn_prefill", "awq_attn_prefill_plan", "awq_rope_with_pos", "awq_rope_neox_inplace"):
        assert hasattr(L, name), name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()
    doc = eng.attn_prefill.__doc__.splitlines()[0]
    params = [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params == ["q", "k", "v", "softmax_scale", "causal"], doc
    # the reference binds these two without keyword names (pybind.cpp:24,29): positional, in the reference's order
    doc = eng.fused_rope_with_pos_forward_func.__doc__.splitlines()[0]
    assert doc.startswith("fused_rope_with_pos_forward_func(arg0: torch.Tensor, arg1: torch.Tensor, arg2: bool)"), doc
    doc = eng.rotary_embedding_neox.__doc__.splitlines()[0]
    assert re.match(r"rotary_embedding_neox\(arg0: torch.Tensor, arg1: torch.Tensor, arg2: torch.Tensor, arg3: [\w.]*Int\w*, arg4: torch.Tensor\)",
                    doc.replace("int,", "Int,")), doc


def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _call(p, **kw):
    a = dict(q=p, k=p, v=p, out=p, B=1, Sq=16, Sk=16, H=8, Hkv=2, Dh=128, qbs=16 * 1024, qrs=1024, kbs=16 * 256, krs=256, vbs=16 * 256,
             vrs=256, scale=0.1, causal=1, dtype=0)
    a.update(kw)
    return _capi.lib().awq_attn_prefill(a["q"], a["k"], a["v"], a["out"], a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"],
                                        a["kbs"], a["krs"], a["vbs"], a["vrs"], a["scale"], a["causal"], a["dtype"], None)


def test_argument_validation_returns_codes_without_launch():
    buf, p = _p16()
    for bad in (dict(Dh=32), dict(Dh=96), dict(Dh=256), dict(H=6, Hkv=4), dict(Sq=17, Sk=16), dict(B=0), dict(Sq=0), dict(Sk=0), dict(H=0),
                dict(Hkv=0)):
        assert _call(p, **bad) == AWQ_ERR_SHAPE, bad
    assert _call(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out"):
        assert _call(p, **{name: None}) == AWQ_ERR_NULL, name
        assert _call(p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 16 * 1024 + 4), ("qrs", 1028), ("kbs", 16 * 256 + 4), ("krs", 260), ("vbs", 16 * 256 + 4), ("vrs", 260)):
        assert _call(p, **{name: val}) == AWQ_ERR_ALIGN, name
    r, n = ctypes.c_int(), ctypes.c_int()
    L = _capi.lib()
    assert L.awq_attn_prefill_plan(1, 8, 2, 96, 16, 16, 1, ctypes.byref(r), ctypes.byref(n)) == AWQ_ERR_SHAPE
    assert L.awq_attn_prefill_plan(1, 8, 2, 128, 17, 16, 1, ctypes.byref(r), ctypes.byref(n)) == AWQ_ERR_SHAPE
    assert L.awq_attn_prefill_plan(1, 8, 2, 128, 17, 16, 0, ctypes.byref(r), ctypes.byref(n)) == 0
    assert L.awq_attn_prefill_plan(1, 8, 2, 128, 16, 16, 1, None, ctypes.byref(n)) == AWQ_ERR_NULL
    # the rope entries: shape, dtype, NULL, alignment
    f = L.awq_rope_with_pos
    ok = dict(n0=2, n1=8, h=4, d=128, d2=128, s0=8 * 512, s1=512, sh=128, o0=8 * 512, o1=512, oh=128, dtype=0)

    def rope(inp=p, fr=p, out=p, **kw):
        a = dict(ok, **kw)
        return f(inp, fr, out, a["n0"], a["n1"], a["h"], a["d"], a["d2"], a["s0"], a["s1"], a["sh"], a["o0"], a["o1"], a["oh"], a["dtype"], None)
    for bad in (dict(d2=136), dict(d2=24), dict(d=100), dict(n0=0), dict(h=0), dict(sh=64)):
        assert rope(**bad) == AWQ_ERR_SHAPE, bad
    assert rope(dtype=2) == AWQ_ERR_DTYPE
    assert rope(inp=None) == AWQ_ERR_NULL and rope(fr=None) == AWQ_ERR_NULL and rope(out=None) == AWQ_ERR_NULL
    assert rope(inp=p + 2) == AWQ_ERR_ALIGN and rope(fr=p + 4) == AWQ_ERR_ALIGN and rope(s1=516) == AWQ_ERR_ALIGN and rope(oh=132) == AWQ_ERR_ALIGN
    g = L.awq_rope_neox_inplace
    assert g(p, p, p, p, 4, 8, 128, 136, 64, 0, None) == AWQ_ERR_SHAPE and g(p, p, p, p, 0, 8, 128, 128, 64, 0, None) == AWQ_ERR_SHAPE
    assert g(p, p, p, p, 4, 8, 128, 128, 64, 2, None) == AWQ_ERR_DTYPE
    assert g(None, p, p, p, 4, 8, 128, 128, 64, 0, None) == AWQ_ERR_NULL and g(p, p, None, p, 4, 8, 128, 128, 64, 0, None) == AWQ_ERR_NULL
    assert g(p + 4, p, p, p, 4, 8, 128, 128, 64, 0, None) == AWQ_ERR_ALIGN and g(p, p + 2, p, p, 4, 8, 128, 128, 64, 0, None) == AWQ_ERR_ALIGN


MODELS = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128), "qwen2_7b": (28, 4, 128), "llama3_70b_tp8": (8, 1, 128)}
# (q_tile_rows, blocks) per (model, Sq, Sk), B = 1, causal: 128 rows; 256 at Dh = 128 once that leaves two blocks per CU; 64 at Dh = 64
# while 128-row tiles leave fewer than two blocks per CU (the choices measured in DESIGN.md "Prefill attention")
PINNED = {
    ("llama3_8b", 16, 16): (128, 32), ("llama3_8b", 256, 256): (128, 64), ("llama3_8b", 1024, 1024): (128, 256),
    ("llama3_8b", 2048, 2048): (128, 512), ("llama3_8b", 4096, 4096): (256, 512), ("llama3_8b", 512, 2560): (128, 128),
    ("llama2_7b", 16, 16): (128, 32), ("llama2_7b", 256, 256): (128, 64), ("llama2_7b", 1024, 1024): (128, 256),
    ("llama2_7b", 2048, 2048): (128, 512), ("llama2_7b", 4096, 4096): (256, 512), ("llama2_7b", 512, 2560): (128, 128),
    ("qwen2_7b", 16, 16): (128, 28), ("qwen2_7b", 256, 256): (128, 56), ("qwen2_7b", 1024, 1024): (128, 224),
    ("qwen2_7b", 2048, 2048): (128, 448), ("qwen2_7b", 4096, 4096): (128, 896), ("qwen2_7b", 512, 2560): (128, 112),
    ("llama3_70b_tp8", 16, 16): (128, 8), ("llama3_70b_tp8", 256, 256): (128, 16), ("llama3_70b_tp8", 1024, 1024): (128, 64),
    ("llama3_70b_tp8", 2048, 2048): (128, 128), ("llama3_70b_tp8", 4096, 4096): (128, 256), ("llama3_70b_tp8", 512, 2560): (128, 32),
}


@pytest.mark.parametrize("key", sorted(PINNED))
def test_plan_is_pinned_and_covers_the_rows(key):
    model, Sq, Sk = key
    H, Hkv, Dh = MODELS[model]
    rows, blocks = ops.attn_prefill_plan(1, H, Hkv, Dh, Sq, Sk, True)
    assert (rows, blocks) == PINNED[key]
    assert rows % 32 == 0 and blocks % H == 0 and (blocks // H) * rows >= Sq > (blocks // H - 1) * rows


def test_plan_of_the_other_head_dim_and_the_widest_tile():
    assert ops.attn_prefill_plan(4, 64, 8, 128, 2048, 2048, True) == (256, 2048)
    assert ops.attn_prefill_plan(1, 64, 8, 64, 256, 256, True) == (64, 256)      # Falcon-like, short prompt
    assert ops.attn_prefill_plan(1, 64, 8, 64, 1024, 1024, True) == (128, 512)
    assert ops.attn_prefill_plan(1, 64, 8, 64, 8192, 8192, True) == (128, 4096)  # Dh = 64 never takes 256 rows


_SHIM = r"""
import sys, importlib.util
real = importlib.util.find_spec("flash_attn") is not None  # (a machine with the CUDA package: it is left alone unless forced)
import llm_awq_amd
if real:
    assert llm_awq_amd.install_as_flash_attn().__name__ == "flash_attn"
    del sys.modules["flash_attn"]
m = llm_awq_amd.install_as_flash_attn(force=real)
from flash_attn import flash_attn_func
import flash_attn
assert flash_attn is m and flash_attn_func is m.flash_attn_func and m.__name__ == "llm_awq_amd.flash_attn_compat"
assert llm_awq_amd.install_as_flash_attn() is m and sys.modules["flash_attn"] is m
other = type(sys)("flash_attn"); sys.modules["flash_attn"] = other
assert llm_awq_amd.install_as_flash_attn() is other          # a flash_attn that is already there is left alone ...
assert llm_awq_amd.install_as_flash_attn(force=True) is m    # ... unless forced
import torch
q = torch.zeros(1, 4, 2, 64, dtype=torch.float16)
for kw, word in ((dict(dropout_p=0.1), "dropout_p"), (dict(window_size=(128, 0)), "window_size"), (dict(alibi_slopes=torch.ones(2)), "alibi_slopes"),
                 (dict(return_attn_probs=True), "return_attn_probs"), (dict(softcap=30.0), "softcap")):
    try:
        flash_attn_func(q, q, q, causal=True, **kw)
    except NotImplementedError as e:
        assert word in str(e), (word, str(e))
    else:
        raise AssertionError(word)
assert not torch.cuda.is_initialized()
try:  # the "off" values pass the keyword check and reach the engine, which refuses CPU tensors
    flash_attn_func(q, q, q, 0.0, None, True, window_size=(-1, -1), alibi_slopes=None, deterministic=True, return_attn_probs=False)
except RuntimeError as e:
    assert not isinstance(e, NotImplementedError) and "GPU" in str(e), str(e)
else:
    raise AssertionError("CPU tensors were accepted")
print("shim ok")
"""


def test_install_as_flash_attn_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-c", _SHIM], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


_TINYCHAT = r"""
import sys, importlib
ref = sys.argv[1]
sys.path.insert(0, ref)
OURS = ("flash_attn", "awq_inference_engine", "llm_awq_amd")

def forget():
    for m in [m for m in sys.modules if m.startswith("tinychat")]:
        del sys.modules[m]

def attempt():
    try:
        return importlib.import_module("tinychat.modules.fused_attn"), None
    except ModuleNotFoundError as e:
        return None, e.name

import llm_awq_amd
# 0. neither name installed: the import fails on one of the two
mod, missing = attempt()
if mod is not None:
    print("SKIP a flash_attn and an awq_inference_engine of the machine's own are importable"); sys.exit(0)
if missing not in ("flash_attn", "awq_inference_engine"):
    print("SKIP", missing); sys.exit(0)  # a third-party package of the reference is not installed here
# 1. the engine alone (fused_attn.py imports it first, :12): what is missing now is flash_attn (:17)
forget()
llm_awq_amd.install_as_awq_inference_engine()
mod, missing = attempt()
if missing is not None and missing.split(".")[0] not in OURS:
    print("SKIP", missing); sys.exit(0)
assert mod is None and missing == "flash_attn", (mod, missing)
# 2. both: the import succeeds; a missing module of ours is a failure, only other packages may skip
forget()
llm_awq_amd.install_as_flash_attn()
mod, missing = attempt()
if missing is not None:
    assert missing.split(".")[0] not in OURS, "still missing after the install calls: " + missing
    print("SKIP", missing); sys.exit(0)
assert mod.flash_attn_func is sys.modules["flash_attn"].flash_attn_func
assert sys.modules["flash_attn"].__name__ == "llm_awq_amd.flash_attn_compat"
print("IMPORT ok")
"""


def test_tinychat_fused_attn_imports_after_the_two_install_calls():
    """Needs a checkout of the reference (llm-awq) named by AWQ_REFERENCE_ROOT whose other imports resolve here."""
    ref = os.environ.get("AWQ_REFERENCE_ROOT")
    if not ref or not os.path.isdir(os.path.join(ref, "tinychat")):
        pytest.skip("AWQ_REFERENCE_ROOT does not name a checkout of the reference")
    r = subprocess.run([sys.executable, "-c", _TINYCHAT, ref], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if "SKIP" in r.stdout:
        pytest.skip("the reference's other imports do not resolve here: " + r.stdout.strip())
    assert "IMPORT ok" in r.stdout


# ------------------------------------------------------------------------------------------------------------------------
# generated code
# ------------------------------------------------------------------------------------------------------------------------
# every instantiation the launch code can reach: 2 dtypes x 2 head dims x {2, 4, 8} waves (the plan runs 4 almost everywhere)
INSTANCES = {(dt, dh, nw): f"attn_prefill_kernelINS_{tag}ELi{dh}ELi{nw}EE" for dt, tag in (("f16", "3F16"), ("bf16", "4BF16")) for dh in (64, 128)
             for nw in (2, 4, 8)}


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
               os.path.join(ROOT, "llm_awq_amd", "csrc"), "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=16",
               "-S", "--cuda-device-only", os.path.join(ROOT, "llm_awq_amd", "csrc", "awq_attn_prefill_cdna4.hip"), "-o", out]
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
def test_generated_code_uses_the_matrix_cores_and_overlaps_its_loads(isa, key):
    body, meta = isa[key]
    dt = key[0]
    assert any(ln.startswith(f"v_mfma_f32_32x32x16_{dt}") for ln in body)
    assert not any(ln.startswith("v_mfma") and f"_{dt}" not in ln for ln in body)
    assert sum(ln.startswith("ds_read_b64_tr_b16") for ln in body) >= 1
    assert ".private_segment_fixed_size: 0" in meta, meta
    assert not any(ln.startswith("scratch_") for ln in body)
    # the tile loop: the back edge that closes over MFMAs.  Inside it, after the last global load of the next K / V tile, at least one
    # MFMA is issued before the first s_waitcnt that names vmcnt
    labels = {m.group(1): i for i, m in ((i, re.match(r"^(\.LBB\d+_\d+):", ln)) for i, ln in enumerate(body)) if m}
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)$", ln)  # (conditional or not: the staging tail may sit behind the loop's test)
        if m and m.group(1) in labels and labels[m.group(1)] < i and any(x.startswith("v_mfma") for x in body[labels[m.group(1)]:i]):
            loops.append((labels[m.group(1)], i))
    assert loops, "no loop with MFMAs"
    lo, hi = min(loops, key=lambda t: t[0])[0], max(loops, key=lambda t: t[1])[1]
    loop = body[lo:hi]
    loads = [i for i, ln in enumerate(loop) if ln.startswith("global_load_dwordx4")]
    assert loads, "the loop does not load the next tile"
    after = loop[loads[-1] + 1:]
    wait = next(i for i, ln in enumerate(after) if ln.startswith("s_waitcnt") and "vmcnt" in ln)
    between = sum(ln.startswith("v_mfma") for ln in after[:wait])
    total = sum(ln.startswith("v_mfma") for ln in loop)
    assert between >= 1, "the loop waits for its loads before any MFMA"
    assert between == total, (between, total)  # in fact the whole tile's MFMAs run under the loads


# ------------------------------------------------------------------------------------------------------------------------
# the needle inputs are sound
# ------------------------------------------------------------------------------------------------------------------------
def _cpu_cases():
    """Every spec whose oracle fits a CPU test (the largest ones are proved sound by their smaller siblings of the same construction)."""
    return [s for s in C.CASES if s["B"] * s["H"] * s["Sq"] * s["Sk"] <= 40_000_000]


def test_case_list_covers_the_axes_of_the_issue():
    names = {s["name"] for s in C.CASES}
    sq = {(s["Sq"], s["Sk"]) for s in C.CASES}
    for S in (1, 2, 63, 64, 65, 127, 129, 1000, 4096):
        assert (S, S) in sq
    for shape in ((1, 500), (130, 700), (512, 2560), (300, 300)):
        assert shape in sq
    assert {s["H"] // s["Hkv"] for s in C.CASES} >= {1, 4, 7, 8} and {s["B"] for s in C.CASES} >= {1, 3}
    assert {s["Dh"] for s in C.CASES} == {64, 128} and {s["dtype"] for s in C.CASES} == {torch.float16, torch.bfloat16}
    assert any(s.get("fused") for s in C.CASES) and any(not s.get("causal", True) for s in C.CASES)
    assert {s.get("mode", "diag") for s in C.CASES} == {"diag", "zero", "scatter", "edges", "decoy", "pair", "negscale"}
    assert {ops.attn_prefill_plan(s["B"], s["H"], s["Hkv"], s["Dh"], s["Sq"], s["Sk"], s.get("causal", True))[0] for s in C.CASES} == {64, 128, 256}
    assert len(names) == len(C.CASES)
    assert len(_cpu_cases()) >= 0.8 * len(C.CASES)


@pytest.mark.parametrize("spec", _cpu_cases(), ids=C.case_id)
def test_oracle_alone_returns_the_targets_and_sees_faults(spec):
    case = C.Case(spec)
    for t in case.backing:  # the padding is NaN, the views are not
        assert torch.isnan(t).any()
    assert not (torch.isnan(case.q).any() or torch.isnan(case.k).any() or torch.isnan(case.v).any())
    out = O.attention(case.q, case.k, case.v, case.scale, case.causal)
    tgt = case.target.double()
    assert float((out - tgt).abs().max()) < 2.0 ** -16
    assert torch.equal(out.to(case.dtype), case.target)
    for mutant in O.MUTANTS:
        if not C.mutant_applies(case, mutant):
            continue
        bad = O.attention(case.q, case.k, case.v, case.scale, case.causal, mutant=mutant)
        assert not torch.equal(bad.to(case.dtype), case.target), mutant


def test_every_fault_is_seen_by_some_case():
    seen = {m: 0 for m in O.MUTANTS}
    for spec in C.CASES:
        if spec["Sq"] > 300:
            continue
        case = C.Case(spec)
        for m in O.MUTANTS:
            seen[m] += C.mutant_applies(case, m)
    assert all(v > 0 for v in seen.values()), seen
