"""The one-row form of the decode GEMV (gemv_dma_kernel_m1, csrc/awq_gemv_dma.hip) is shaped by how many instructions a wave issues per
128-k step and in which order; hipcc decides both, so this test reads the GENERATED gfx950 ISA of the three bf16 sz_half instantiations one
decoded Llama-3-8B token runs (gate/up: 8 waves, ring 4, EPI 2; down_proj: 16 waves, ring 1; o_proj: 8 waves, ring 2) and checks what the
form was built for (profiles/decode_step_pipeline.txt):

  * head: no branch between the first `buffer_load ... lds` and the first counted `s_waitcnt vmcnt` -- the up-front DMAs are a straight line;
  * step: 12 MFMAs (8 dequant, 4 product) and at most 41 other v_* instructions (the arithmetic needs 39: 16 v_and_or, 16 v_cvt_pk, 4 v_lshrrev,
    2 v_perm, 1 for the offset sz - 1024 s; the parent commit's loop spent 46);
  * pipeline: in every step but the last, four ds_read_b128 and one ds_read_b32 of the FOLLOWING step are issued before the step's last
    product MFMA;
  * the compiler's occupancy estimate stays >= 6 waves per SIMD (gate/up runs three 8-wave blocks per CU);
  * no dequant MFMA directly behind an inline-asm VALU write of one of its operands (hipcc's hazard recogniser does not look inside asm).

A step is what lies between two `s_waitcnt lgkmcnt(0)` -- the wait that hands a step its weight tile; the last step ends with its last
product MFMA.  CPU-only (hipcc cross-compiles gfx950); one compilation for the module."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# template arguments <DT, WAVES, D, DQ, EPI, TX> as they appear in the mangled name, and the steps each wave runs
KERNELS = {
    "gate_up": ("gemv_dma_kernel_m1INS_4BF16ELi8ELi4ELi1ELi2ELi4EE", 4),
    "down": ("gemv_dma_kernel_m1INS_4BF16ELi16ELi1ELi1ELi0ELi7EE", 7),
    "o": ("gemv_dma_kernel_m1INS_4BF16ELi8ELi2ELi1ELi0ELi4EE", 4),
}


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        # the flags of llm_awq_amd/build.py
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
               os.path.join(ROOT, "llm_awq_amd", "csrc"), "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=16",
               "-S", "--cuda-device-only", os.path.join(ROOT, "llm_awq_amd", "csrc", "awq_gemv_dma.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        text = open(out).read().split("\n")
    found = {}
    for name, (key, steps) in KERNELS.items():
        starts = [i for i, ln in enumerate(text) if ln.startswith("_ZN3awq") and key in ln.split(":")[0] and ln.split(":")[0].endswith("iiiii")]
        if len(starts) != 1:
            continue
        s = starts[0]
        e = next(i for i in range(s, len(text)) if text[i].strip().startswith(".size"))
        body = [ln.strip() for ln in text[s + 1:e]]
        body = [ln for ln in body if ln and not ln.startswith(";") and not ln.startswith(".") and "ASMSTART" not in ln and "ASMEND" not in ln]
        occ = next(int(m.group(1)) for m in (re.match(r"\s*; Occupancy: (\d+)", ln) for ln in text[e:e + 80]) if m)
        found[name] = (body, occ, steps)
    return found


def _steps(body):
    """-> (index of the first DMA, index of the first counted vmcnt wait, [instructions of step 0, 1, ...])"""
    first_dma = next(i for i, ln in enumerate(body) if ln.startswith("buffer_load") and ln.endswith(" lds"))
    first_vm = next(i for i, ln in enumerate(body) if ln.startswith("s_waitcnt vmcnt("))
    barrier = next(i for i, ln in enumerate(body) if ln.startswith("s_barrier"))
    last_product = max(i for i in range(first_vm, barrier) if body[i].startswith("v_mfma_f32_16x16x32"))
    cuts = [i for i in range(first_vm, last_product) if body[i].startswith("s_waitcnt lgkmcnt(0)")]
    segs = [body[a + 1:b] for a, b in zip(cuts, cuts[1:] + [last_product + 1])]
    return first_dma, first_vm, [sg for sg in segs if any(ln.startswith("v_mfma") for ln in sg)]


def test_all_three_instantiations_are_there(isa):
    assert sorted(isa) == sorted(KERNELS), sorted(isa)
    for name, (body, _occ, steps) in isa.items():
        assert len(_steps(body)[2]) == steps, (name, len(_steps(body)[2]))


def test_head_is_a_straight_line(isa):
    assert len(isa) == 3
    for name, (body, _occ, _steps_n) in isa.items():
        first_dma, first_vm, _ = _steps(body)
        head = body[first_dma:first_vm]
        assert first_dma < first_vm, name
        assert sum(ln.startswith("buffer_load") for ln in head) >= 4, (name, head)  # tile 0, scales, x, (the rest of the ring)
        assert not [ln for ln in head if ln.startswith("s_cbranch") or ln.startswith("s_branch")], (name, head)


def test_step_instruction_budget(isa):
    assert len(isa) == 3
    for name, (body, _occ, _steps_n) in isa.items():
        for t, seg in enumerate(_steps(body)[2]):
            mfma = [ln for ln in seg if ln.startswith("v_mfma")]
            valu = [ln for ln in seg if ln.startswith("v_") and not ln.startswith("v_mfma")]
            assert len(mfma) == 12, (name, t, len(mfma))
            assert len(valu) <= 41, (name, t, len(valu), valu)


def test_next_step_reads_are_issued_under_the_math(isa):
    assert len(isa) == 3
    for name, (body, _occ, _steps_n) in isa.items():
        segs = _steps(body)[2]
        for t, seg in enumerate(segs[:-1]):
            last_product = max(j for j, ln in enumerate(seg) if ln.startswith("v_mfma_f32_16x16x32"))
            ahead = seg[:last_product]
            assert sum(ln.startswith("ds_read_b128") for ln in ahead) >= 4, (name, t)
            assert sum(ln.startswith("ds_read_b32") for ln in ahead) >= 1, (name, t)


def test_occupancy(isa):
    assert len(isa) == 3
    for name, (_body, occ, _steps_n) in isa.items():
        assert occ >= 6, (name, occ)


def test_no_asm_valu_write_directly_in_front_of_the_mfma_that_reads_it(isa):
    def regs(tok):
        m = re.match(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return {int(m.group(1))} if m else set()

    assert len(isa) == 3
    checked = 0
    for name, (body, _occ, _steps_n) in isa.items():
        for i, ln in enumerate(body):
            if not ln.startswith("v_mfma"):
                continue
            checked += 1
            srcs = set()
            for tok in [t.strip() for t in ln.split(None, 1)[1].split(",")][1:]:
                srcs |= regs(tok)
            j, wait = i - 1, 0
            while j >= 0 and body[j].startswith("s_nop"):
                wait += int(body[j].split()[1]) + 1
                j -= 1
            prev = body[j]
            if prev.startswith("v_mov_b64") and wait < 2:  # the instruction Cdna4DequantH::prep_lean issues from asm
                assert not (regs(prev.split(None, 1)[1].split(",")[0].strip()) & srcs), (name, prev, ln)
    assert checked >= 12 * (4 + 7 + 4), checked
