"""Split-KV attention without a GPU: the exports, the host plan's fixed conditions and pinned values, the workspace formula, the knob, the
C ABI's argument checks (csrc/awq_attn_splitkv_cdna4.hip, awq_rope_kv_store_natural), and the soundness of the needle inputs of
tests/attn_splitkv_oracle.py -- the list tests/test_gpu_attention_splitkv.py runs through the kernels -- against the torch restatement
of split-and-combine and each of its mutants."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

import llm_awq_amd
from llm_awq_amd import _capi, ops
from tests import attn_prefill_cases as C
from tests import attn_prefill_oracle as O
from tests import attn_splitkv_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
AWQ_ERR_DTYPE, AWQ_ERR_SHAPE, AWQ_ERR_ALIGN, AWQ_ERR_NULL, AWQ_ERR_WORKSPACE = -3, -4, -5, -6, -7
KCUS = 256


def test_library_engine_and_ops_export_the_splitkv_surface():
    L = _capi.lib()
    for name in ("awq_attn_splitkv", "awq_attn_splitkv_plan", "awq_attn_splitkv_workspace_bytes", "awq_rope_kv_store_natural"):
        assert hasattr(L, name), name
    assert L.awq_abi_version() == 1
    eng = llm_awq_amd.load_engine()

    def params(fn):
        doc = fn.__doc__.splitlines()[0]
        return [p.split(":")[0].strip() for p in doc[doc.index("(") + 1:doc.rindex(")")].split(", ")]
    assert params(eng.attn_splitkv) == ["q", "k", "v", "softmax_scale", "causal"]
    assert params(eng.attn_splitkv_plan) == ["batch", "nheads", "nheads_kv", "head_dim", "seqlen_q", "seqlen_k", "causal"]
    assert params(eng.rope_kv_store_natural) == ["qkv", "freqs", "k_cache", "v_cache", "start_pos", "nheads", "nheads_kv"]
    assert params(eng.attn_prefill) == ["q", "k", "v", "softmax_scale", "causal"]  # the one-pass export is still there
    for name in ("attn_splitkv_plan", "attn_splitkv", "rope_kv_store_natural"):
        assert callable(getattr(ops, name)), name
    assert eng.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True)


# ------------------------------------------------------------------------------------------------------------------------
# the plan
# ------------------------------------------------------------------------------------------------------------------------
MODELS = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128), "qwen2_7b": (28, 4, 128), "llama3_70b_tp8": (8, 1, 128)}
GRID = [(m, B, Sq, Sk) for m in sorted(MODELS) for B in (1, 8) for Sq in (1, 8, 32, 33, 129) for Sk in (1, 2047, 2048, 2049, 32768, 131072)]


def _ws(B, H, Hkv, Dh, Sq, Sk, causal):
    return _capi.lib().awq_attn_splitkv_workspace_bytes(B, H, Hkv, Dh, Sq, Sk, int(causal))


@pytest.mark.parametrize("model,B,Sq,Sk", GRID, ids=lambda x: str(x))
def test_plan_keeps_the_fixed_conditions(model, B, Sq, Sk):
    H, Hkv, Dh = MODELS[model]
    G = H // Hkv
    causal = Sq <= Sk  # (a causal call needs Sq <= Sk; the remaining points are asked without a mask)
    splits, chunk = ops.attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, causal)
    one_pass_blocks = ops.attn_prefill_plan(B, H, Hkv, Dh, Sq, Sk, causal)[1]
    if Sk < 2048 or Sq * G > 128 or one_pass_blocks >= KCUS:
        assert splits == 1
        assert _ws(B, H, Hkv, Dh, Sq, Sk, causal) == 0
        return
    assert splits > 1
    assert chunk % 64 == 0 and chunk >= 1024
    assert (splits - 1) * chunk < Sk <= splits * chunk
    if B * Hkv * (Sk // 1024) >= KCUS:
        assert B * Hkv * splits >= KCUS
    assert _ws(B, H, Hkv, Dh, Sq, Sk, causal) == B * H * Sq * splits * (Dh + 2) * 4


def test_plan_never_splits_other_head_dims_and_answers_both_masks():
    assert ops.attn_splitkv_plan(1, 16, 16, 72, 1, 32768, False)[0] == 1   # the tower head dim: the one-pass form
    assert ops.attn_splitkv_plan(1, 32, 8, 64, 1, 32768, True)[0] > 1
    assert ops.attn_splitkv_plan(1, 32, 8, 64, 1, 32768, False) == ops.attn_splitkv_plan(1, 32, 8, 64, 1, 32768, True)
    s, c = ctypes.c_int(), ctypes.c_int()
    L = _capi.lib()
    assert L.awq_attn_splitkv_plan(1, 32, 8, 96, 1, 4096, 1, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_splitkv_plan(1, 32, 8, 128, 5, 4, 1, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_splitkv_plan(1, 32, 6, 128, 1, 4096, 1, ctypes.byref(s), ctypes.byref(c)) == AWQ_ERR_SHAPE
    assert L.awq_attn_splitkv_plan(1, 32, 8, 128, 1, 4096, 1, None, ctypes.byref(c)) == AWQ_ERR_NULL
    assert L.awq_attn_splitkv_plan(1, 32, 8, 128, 1, 4096, 1, ctypes.byref(s), None) == AWQ_ERR_NULL
    assert L.awq_attn_splitkv_workspace_bytes(1, 32, 8, 96, 1, 4096, 1) == 0


# (splits, chunk) per (model, B, Sq, Sk), causal: the rule of attn_splitkv_plan as it stands (two blocks per CU, chunks >= 1024; not measured)
PINNED = {
    ("llama3_8b", 1, 1, 2048): (2, 1024), ("llama3_8b", 1, 1, 2049): (3, 1024), ("llama3_8b", 1, 1, 8192): (8, 1024),
    ("llama3_8b", 1, 1, 32768): (32, 1024), ("llama3_8b", 1, 1, 131072): (64, 2048), ("llama3_8b", 1, 8, 32768): (32, 1024),
    ("llama3_8b", 8, 1, 32768): (1, 32768), ("llama3_8b", 8, 1, 131072): (1, 131072),  # 256 one-pass blocks already
    ("llama3_70b_tp8", 8, 1, 32768): (32, 1024),
    ("llama2_7b", 1, 1, 32768): (16, 2048), ("llama2_7b", 8, 1, 32768): (1, 32768),
    ("qwen2_7b", 1, 1, 32768): (32, 1024), ("qwen2_7b", 1, 1, 131072): (128, 1024), ("qwen2_7b", 1, 8, 2049): (3, 1024),
    ("llama3_70b_tp8", 1, 1, 131072): (128, 1024), ("llama3_70b_tp8", 8, 8, 131072): (64, 2048), ("llama3_70b_tp8", 1, 32, 2048): (1, 2048),
}


@pytest.mark.parametrize("key", sorted(PINNED))
def test_plan_is_pinned(key):
    model, B, Sq, Sk = key
    H, Hkv, Dh = MODELS[model]
    assert ops.attn_splitkv_plan(B, H, Hkv, Dh, Sq, Sk, True) == PINNED[key]


@pytest.fixture
def knob():
    had = os.environ.get("AWQ_TUNING")
    yield lambda c: _capi.tune(attn_splitkv_chunk=c)
    _capi.tune(attn_splitkv_chunk=0)
    if had is None:
        os.environ.pop("AWQ_TUNING", None)


def test_knob_forces_the_chunk_and_the_workspace_follows(knob):
    L = _capi.lib()
    before = ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True)
    knob(64)
    assert ops.attn_splitkv_plan(1, 8, 2, 128, 8, 193, True) == (4, 64)       # any Sk
    assert ops.attn_splitkv_plan(1, 8, 2, 128, 1, 64, True) == (1, 64)        # one chunk: the one-pass kernel
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == (512, 64)
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 33, 193, True)[0] == 1        # Sq * G = 132 > 128 still holds
    assert ops.attn_splitkv_plan(1, 16, 16, 72, 8, 193, False)[0] == 1        # .. and the head dim
    assert _ws(1, 8, 2, 128, 8, 193, True) == 1 * 8 * 8 * 4 * 130 * 4
    assert _ws(1, 8, 2, 128, 1, 64, True) == 0
    knob(4096)
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == (8, 4096)
    assert L.awq_tune_set(b"attn_splitkv_chunk", 100) == AWQ_ERR_SHAPE        # not a multiple of 64: refused, nothing changes
    assert L.awq_tune_set(b"attn_splitkv_chunk", -64) == AWQ_ERR_SHAPE
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == (8, 4096)
    knob(0)
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == before
    # inert without AWQ_TUNING=1
    os.environ.pop("AWQ_TUNING", None)
    assert L.awq_tune_set(b"attn_splitkv_chunk", 64) == AWQ_ERR_SHAPE
    assert ops.attn_splitkv_plan(1, 32, 8, 128, 1, 32768, True) == before


# ------------------------------------------------------------------------------------------------------------------------
# argument validation: every code, no GPU call
# ------------------------------------------------------------------------------------------------------------------------
def _p16():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _call(p, **kw):
    # Sk = 4096, Sq * G = 4: the plan splits, so a valid call would need the workspace -- which stays NULL: nothing is ever launched
    a = dict(q=p, k=p, v=p, out=p, B=1, Sq=1, Sk=4096, H=8, Hkv=2, Dh=128, qbs=1024, qrs=1024, kbs=4096 * 256, krs=256, vbs=4096 * 256,
             vrs=256, scale=0.1, causal=1, dtype=0, ws=None, wsb=0)
    a.update(kw)
    return _capi.lib().awq_attn_splitkv(a["q"], a["k"], a["v"], a["out"], a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["Dh"], a["qbs"], a["qrs"],
                                        a["kbs"], a["krs"], a["vbs"], a["vrs"], a["scale"], a["causal"], a["dtype"], a["ws"], a["wsb"], None)


def test_splitkv_argument_validation_returns_codes_without_launch():
    buf, p = _p16()
    for bad in (dict(Dh=32), dict(Dh=96), dict(Dh=256), dict(H=6, Hkv=4), dict(Sq=4097), dict(B=0), dict(Sq=0), dict(Sk=0), dict(H=0),
                dict(Hkv=0), dict(qrs=512), dict(krs=128), dict(vrs=128), dict(qbs=-8), dict(Dh=72)):
        assert _call(p, **bad) == AWQ_ERR_SHAPE, bad
    assert _call(p, dtype=2) == AWQ_ERR_DTYPE
    for name in ("q", "k", "v", "out"):
        assert _call(p, **{name: None}) == AWQ_ERR_NULL, name
        assert _call(p, **{name: p + 2}) == AWQ_ERR_ALIGN, name
    for name, val in (("qbs", 1028), ("qrs", 1028), ("kbs", 4096 * 256 + 4), ("krs", 260), ("vbs", 4096 * 256 + 4), ("vrs", 260)):
        assert _call(p, **{name: val}) == AWQ_ERR_ALIGN, name
    need = _ws(1, 8, 2, 128, 1, 4096, True)
    assert need == 1 * 8 * 1 * ops.attn_splitkv_plan(1, 8, 2, 128, 1, 4096, True)[0] * 130 * 4 > 0
    assert _call(p) == AWQ_ERR_WORKSPACE                       # the plan splits: a workspace is needed
    assert _call(p, ws=p, wsb=need - 1) == AWQ_ERR_WORKSPACE
    assert _call(p, ws=None, wsb=need) == AWQ_ERR_WORKSPACE
    assert _call(p, ws=p + 4, wsb=need) == AWQ_ERR_ALIGN


def test_rope_kv_store_natural_argument_validation_returns_codes_without_launch():
    buf, p = _p16()
    f = _capi.lib().awq_rope_kv_store_natural
    ok = dict(qkv=p, fr=p, q=p, kc=p, vc=p, B=1, Bc=2, S=4, H=8, Hkv=2, Dh=128, rot=128, lmax=64, start=3, bs=4 * 1536, rs=1536, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["qkv"], a["fr"], a["q"], a["kc"], a["vc"], a["B"], a["Bc"], a["S"], a["H"], a["Hkv"], a["Dh"], a["rot"], a["lmax"], a["start"],
                 a["bs"], a["rs"], a["dtype"], None)
    for bad in (dict(Dh=96), dict(Dh=72), dict(rot=24), dict(rot=144), dict(rot=0), dict(B=3), dict(B=0), dict(S=0), dict(H=0), dict(Hkv=0),
                dict(start=-1), dict(start=61), dict(lmax=0), dict(rs=1528), dict(bs=-8)):
        assert call(**bad) == AWQ_ERR_SHAPE, bad
    assert call(dtype=2) == AWQ_ERR_DTYPE
    for name in ("qkv", "fr", "q", "kc", "vc"):
        assert call(**{name: None}) == AWQ_ERR_NULL, name
        assert call(**{name: p + 4}) == AWQ_ERR_ALIGN, name
    assert call(bs=4 * 1536 + 4) == AWQ_ERR_ALIGN and call(rs=1540) == AWQ_ERR_ALIGN


def test_flash_attn_shim_keeps_its_keyword_handling():
    from llm_awq_amd import flash_attn_compat as F

    q = torch.zeros(1, 1, 8, 128, dtype=torch.float16)
    k = torch.zeros(1, 4096, 2, 128, dtype=torch.float16)
    for kw, word in ((dict(dropout_p=0.1), "dropout_p"), (dict(window_size=(128, 0)), "window_size"), (dict(softcap=30.0), "softcap"),
                     (dict(alibi_slopes=torch.ones(8)), "alibi_slopes"), (dict(return_attn_probs=True), "return_attn_probs")):
        with pytest.raises(NotImplementedError, match=word):
            F.flash_attn_func(q, k, k, causal=True, **kw)
    with pytest.raises(RuntimeError, match="GPU") as e:  # a split-routed shape on the CPU reaches the engine, which refuses it
        F.flash_attn_func(q, k, k, causal=True, window_size=(-1, -1), deterministic=True)
    assert not isinstance(e.value, NotImplementedError)


# ------------------------------------------------------------------------------------------------------------------------
# generated code (the manner of tests/test_attention_prefill_host.py)
# ------------------------------------------------------------------------------------------------------------------------
INSTANCES = {(dt, dh): f"attn_splitkv_kernelINS_{tag}ELi{dh}EE" for dt, tag in (("f16", "3F16"), ("bf16", "4BF16")) for dh in (64, 128)}


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
               os.path.join(ROOT, "llm_awq_amd", "csrc"), "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=16",
               "-S", "--cuda-device-only", os.path.join(ROOT, "llm_awq_amd", "csrc", "awq_attn_splitkv_cdna4.hip"), "-o", out]
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
        ind = len(text[meta]) - len(text[meta].lstrip())
        top = lambda j: text[j].startswith(" " * (ind - 2) + "- .")
        lo = max(j for j in range(meta + 1) if top(j))
        hi = next((j for j in range(meta + 1, len(text)) if top(j) or not text[j].startswith(" " * (ind - 2))), len(text))
        found[key] = (body, "\n".join(text[lo:hi]))
    return found


@pytest.mark.parametrize("key", sorted(INSTANCES))
def test_generated_code_uses_the_matrix_cores_and_overlaps_its_loads(isa, key):
    body, meta = isa[key]
    dt, dh = key
    assert sum(ln.startswith(f"v_mfma_f32_32x32x16_{dt}") for ln in body) == dh // 4  # one 64-key tile: 2 Dh / 16 for S, 4 Dh / 32 for O
    assert not any(ln.startswith("v_mfma") and f"_{dt}" not in ln for ln in body)
    assert sum(ln.startswith("ds_read_b64_tr_b16") for ln in body) >= 1
    assert ".private_segment_fixed_size: 0" in meta, meta
    assert f".group_segment_fixed_size: {4 * 64 * dh * 2}" in meta, meta  # K and V, double-buffered: two blocks per CU at Dh = 128
    assert not any(ln.startswith("scratch_") for ln in body)
    assert not any("atomic" in ln for ln in body)
    # the tile loop: after the last global load of the next K / V tile every MFMA of the tile is issued before the first wait on vmcnt
    labels = {m.group(1): i for i, m in ((i, re.match(r"^(\.LBB\d+_\d+):", ln)) for i, ln in enumerate(body)) if m}
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)$", ln)
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
    assert between == total >= 1, (between, total)


# ------------------------------------------------------------------------------------------------------------------------
# the needle inputs are sound, and every mutant of the restatement is seen
# ------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_axes_of_the_issue():
    names = {s["name"] for s in S.CASES}
    assert len(names) == len(S.CASES)
    assert {(s["Sq"], s["Sk"]) for s in S.CASES} == {(1, 65), (1, 129), (8, 193), (32, 257)}
    assert {s["H"] // s["Hkv"] for s in S.CASES} >= {1, 4, 7, 8} and {s["B"] for s in S.CASES} >= {1, 3}
    assert {s["Dh"] for s in S.CASES} == {64, 128} and {s["dtype"] for s in S.CASES} == {torch.float16, torch.bfloat16}
    assert any(s.get("fused") for s in S.CASES) and any(not s.get("causal", True) for s in S.CASES)
    assert all(s["Sq"] * (s["H"] // s["Hkv"]) <= 128 for s in S.CASES)
    for Sq, Sk in S.SHAPES:  # every shape meets every group size it can serve, both batches and a KV head count above one
        mine = [s for s in S.CASES if (s["Sq"], s["Sk"]) == (Sq, Sk)]
        assert {s["H"] // s["Hkv"] for s in mine} >= {g for g in (1, 4, 7, 8) if Sq * g <= 128}
        assert {s["B"] for s in mine} >= {1, 3} and {s["Dh"] for s in mine} == {64, 128} and any(s["Hkv"] > 1 for s in mine)


@pytest.mark.parametrize("spec", S.CASES, ids=S.case_id)
def test_restatement_returns_the_targets_and_every_mutant_is_seen(spec):
    case = C.Case(spec)
    assert not (torch.isnan(case.q).any() or torch.isnan(case.k).any() or torch.isnan(case.v).any())
    # the float64 oracle first: the inputs are sound whatever the split
    ref = O.attention(case.q, case.k, case.v, case.scale, case.causal)
    assert torch.equal(ref.to(case.dtype), case.target)
    for chunk in (S.CHUNK, 128):  # the target does not depend on how the keys are cut
        out = S.splitkv(case.q, case.k, case.v, case.scale, case.causal, chunk=chunk)
        assert torch.equal(out.view(torch.int16), case.target.view(torch.int16)), chunk
    for mutant in S.MUTANTS:
        if not S.mutant_applies(case, mutant):
            continue
        bad = S.splitkv(case.q, case.k, case.v, case.scale, case.causal, chunk=S.CHUNK, mutant=mutant)
        assert not torch.equal(bad.view(torch.int16), case.target.view(torch.int16)), mutant


def test_every_mutant_is_seen_by_some_case_of_every_shape_it_can_show_at():
    for Sq, Sk in S.SHAPES:
        seen = {m: 0 for m in S.MUTANTS}
        for spec in S.CASES:
            if (spec["Sq"], spec["Sk"]) == (Sq, Sk):
                case = C.Case(spec)
                for m in S.MUTANTS:
                    seen[m] += S.mutant_applies(case, m)
        cannot = {"mask+1", "emptynan", "rowpack"} if Sq == 1 else set()  # one query row: nothing masked, no empty split, nothing to permute
        assert all(v > 0 for m, v in seen.items() if m not in cannot), ((Sq, Sk), seen)


def test_the_empty_split_case_of_the_issue_is_in_the_list():
    """Sq = 8, Sk = 3 * 64 + 1, chunk 64: the last chunk holds one key and rows 0 .. 6 attend nothing of it."""
    spec = next(s for s in S.CASES if s["name"].startswith("diag-8x193-G4"))
    assert S.split_ranges(193, 64)[-1] == (192, 193)
    case = C.Case(spec)
    assert (case.lim[:7] < 192).all() and case.lim[7] == 192
    bad = S.splitkv(case.q, case.k, case.v, case.scale, True, chunk=64, mutant="emptynan")
    assert torch.isnan(bad.float()[:, :7]).all() and not torch.isnan(bad.float()[:, 7]).any()
    out = S.splitkv(case.q, case.k, case.v, case.scale, True, chunk=64)
    assert torch.isfinite(out.float()).all()
