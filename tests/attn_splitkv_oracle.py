"""Split-KV attention restated in torch on the CPU, the way csrc/awq_attn_splitkv_cdna4.hip computes it, and the needle inputs its tests share.

    per (batch, KV head): the Sq * G query rows of the group are packed, row = i * G + g
    per split s (keys [s * chunk, min(Sk, (s + 1) * chunk))): base-2 logits in fp32, masked; m_s = their max; every weight
        2^(x - m_s) rounded to T ONCE, that rounded value feeding both l_s = sum p and O_s = p V (fp32, unnormalised);
        a row that attends nothing of the split: O_s = 0, l_s = 0, m_s = -inf
    combine: M = max_s m_s; O = sum_s 2^(m_s - M) O_s, L = sum_s 2^(m_s - M) l_s in ascending split order, a split with m_s = -inf
        skipped; out = T(O * (1 / L)): one division, one rounding

(The kernel walks a split in 64-key tiles with a running max; the restatement takes the split's max at once.  On the needle inputs both
are exact -- that is what the needles are for -- and on random inputs the float64 oracle of tests/attn_prefill_oracle.py is the judge.)

`mutant` switches one fault in, for the tests that prove the needle inputs can see it:
    dropsplit         the last split is not combined
    norescale         the partials are added without their 2^(m_s - M) weights
    edge+1 / edge-1   every split after the first begins one key early / late: a boundary key is visited twice / not at all
    mask+1 / mask-1   the causal limit moved by one in either direction
    kvh+1             the next KV head
    emptynan          a partial that attended nothing is neither zeroed nor skipped (2^(-inf + inf))
    rowpack           the packed rows are unpacked as row = g * Sq + i instead of i * G + g
"""
from __future__ import annotations

import torch

from tests.attn_prefill_oracle import bound as _one_pass_bound

MUTANTS = ("dropsplit", "norescale", "edge+1", "edge-1", "mask+1", "mask-1", "kvh+1", "emptynan", "rowpack")
LOG2E = 1.4426950408889634


def split_ranges(Sk: int, chunk: int, mutant=None):
    """[begin, end) of every split, as the launch code states it."""
    out = []
    for s in range((Sk + chunk - 1) // chunk):
        lo = s * chunk
        if s > 0:
            lo += {"edge+1": -1, "edge-1": 1}.get(mutant, 0)
        out.append((lo, min(Sk, (s + 1) * chunk)))
    return out


def splitkv(q, k, v, scale=None, causal=False, chunk: int = 64, mutant=None):
    """q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] of dtype T (CPU) -> out T [B, Sq, H, Dh]."""
    assert chunk % 64 == 0
    B, Sq, H, Dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = H // Hkv
    R = Sq * G
    T = q.dtype
    f32 = torch.float32
    sc = torch.tensor((float(Dh) ** -0.5 if scale is None else float(scale)), dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    shift = Sk - Sq + {"mask+1": 1, "mask-1": -1}.get(mutant, 0)
    ranges = split_ranges(Sk, chunk, mutant)
    out = torch.empty(B, Sq, H, Dh, dtype=T)
    rows = torch.arange(R)
    qi, qg = rows // G, rows % G  # packed row = i * G + g
    ninf = float("-inf")
    for b in range(B):
        for kvh in range(Hkv):
            src = (kvh + 1) % Hkv if mutant == "kvh+1" else kvh
            Q = q[b, qi, kvh * G + qg].to(f32)  # [R, Dh]
            part = []
            for lo, hi in ranges:
                if hi <= lo:  # (edge-1 on a one-key split: nothing left of it)
                    part.append((torch.zeros(R, Dh, dtype=f32), torch.full((R,), ninf, dtype=f32), torch.zeros(R, dtype=f32)))
                    continue
                K, V = k[b, lo:hi, src].to(f32), v[b, lo:hi, src].to(f32)
                x = (Q @ K.T) * sc
                if causal:
                    x = x.masked_fill(torch.arange(lo, hi)[None, :] > (qi + shift)[:, None], ninf)
                m = x.max(-1).values  # [R]
                if mutant == "emptynan":
                    p = torch.exp2(x - m[:, None]).to(T).to(f32)  # -inf - -inf
                else:
                    p = torch.exp2(x - torch.where(m == ninf, torch.zeros_like(m), m)[:, None]).to(T).to(f32)
                part.append((p @ V, m, p.sum(-1)))
            if mutant == "dropsplit":
                part = part[:-1]
            M = torch.stack([m for _, m, _ in part]).max(0).values
            acc, L = torch.zeros(R, Dh, dtype=f32), torch.zeros(R, dtype=f32)
            for O, m, l in part:
                w = torch.ones_like(m) if mutant == "norescale" else torch.exp2(m - M)
                live = (m != ninf) | (mutant == "emptynan")
                acc = torch.where(live[:, None], w[:, None] * O + acc, acc)
                L = torch.where(live, w * l + L, L)
            res = (acc * (1.0 / L)[:, None]).to(T)  # [R, Dh]
            if mutant == "rowpack":
                out[b, rows % Sq, kvh * G + rows // Sq] = res
            else:
                out[b, qi, kvh * G + qg] = res
    return out


def bound(ref, Aw, qk, dtype, Sk, Dh, scale, splits):
    """tests.attn_prefill_oracle.bound plus the combine term.

    Inside a split the kernel is the flash loop that bound describes (fp32 scores and accumulation, weights rounded to T once), over
    at most `chunk` <= Sk keys; out = (sum_s w_s O_s) / (sum_s w_s l_s), w_s = 2^(m_s - M), is a weighted mean of the per-split results
    with weights w_s l_s / L that add up to 1, so the per-split errors combine to at most that bound with Sk keys.  The combine adds:
      * the two fp32 sums over the splits, one fmaf each per split: at most splits * 2^-24 relative on the numerator (whose terms are
        bounded by L A) and on the denominator: 2 splits 2^-24 A;
      * the weights: w_s carries the rounding of m_s - M (|m_s - M| 2^-24 absolute, times ln 2 in the exponent) and of exp2 (one ulp,
        2^-23): delta_s <= (2 + 0.7 d_s) 2^-24 with d_s = M - m_s.  The same w_s multiplies O_s and l_s, so only the SHIFT of weight
        between the splits shows: sum_s delta_s (w_s l_s / L) (A_s + A) <= 2 max_s delta_s A, because sum_s (w_s l_s / L) A_s = A.  A
        split with d_s > 40 weighs w_s l_s / L <= 2^-40 Sk and cannot show; for the others delta_s <= 30 * 2^-24: 60 * 2^-24 A.
    Together (2 splits + 60) 2^-24 A: small against the 2 Sk 2^-24 A the one-pass bound already grants the sums over the keys (splits <= Sk / 1024
    under the plan)."""
    return _one_pass_bound(ref, Aw, qk, dtype, Sk, Dh, scale) + (2 * splits + 60) * 2.0 ** -24 * Aw


# ------------------------------------------------------------------------------------------------------------------------
# needle inputs: tests.attn_prefill_cases.Case specs (imported there, not edited) at the smallest shapes where each fault shows, for a
# forced chunk of 64 keys.  Every mode of Case is one-hot (or an exact mean of two rows), so its target does not depend on how the keys
# are cut: tests/test_attention_splitkv_host.py checks on the CPU that the restatement above reproduces every target bit for bit.
# ------------------------------------------------------------------------------------------------------------------------
CHUNK = 64
SHAPES = ((1, 65), (1, 129), (8, 193), (32, 257))  # (8, 193): the last chunk holds ONE key and rows 0 .. 6 attend nothing of it


def _cases():
    out = []

    def add(name, **kw):
        for dt in (torch.float16, torch.bfloat16):
            out.append(dict(kw, name=f"{name}-{str(dt)[6:]}", dtype=dt))

    n = 0
    for Sq, Sk in SHAPES:
        for G in (1, 4, 7, 8):
            if Sq * G > 128:  # not served by the split kernel
                continue
            # B, Dh and Hkv take turns; every (Sq, Sk) meets B = 1 and 3, both head dims and Hkv > 1
            B, Dh, Hkv = (1, 3)[n % 2], (64, 128)[(n // 2) % 2], (2, 1, 3)[n % 3]
            add(f"diag-{Sq}x{Sk}-G{G}", B=B, H=G * Hkv, Hkv=Hkv, Dh=Dh, Sq=Sq, Sk=Sk, mode="diag", fused=(G == 4 and Sq == 8))
            n += 1
        Dh = (128, 64)[n % 2]
        add(f"pair-edge-{Sq}x{Sk}", B=1, H=4, Hkv=2, Dh=Dh, Sq=Sq, Sk=Sk, mode="pair", pair=(63, 64))  # both sides of the first split edge
        add(f"edges-{Sq}x{Sk}", B=1, H=4, Hkv=1, Dh=128 + 64 - Dh, Sq=Sq, Sk=Sk, mode="edges")
        add(f"scatter-{Sq}x{Sk}", B=3, H=4, Hkv=2, Dh=Dh, Sq=Sq, Sk=Sk, mode="scatter", fused=(Sq == 1 and Sk == 129))
        add(f"negscale-{Sq}x{Sk}", B=1, H=2, Hkv=2, Dh=128 + 64 - Dh, Sq=Sq, Sk=Sk, mode="negscale")
        if Sq > 1:  # (one query row has no masked key to put a decoy on)
            for c in range(3):
                add(f"decoy{c}-{Sq}x{Sk}", B=1, H=2, Hkv=1, Dh=Dh, Sq=Sq, Sk=Sk, mode="decoy", call=c)
        if Sk > 128:
            add(f"pair-edge2-{Sq}x{Sk}", B=1, H=2, Hkv=1, Dh=Dh, Sq=Sq, Sk=Sk, mode="pair", pair=(127, 128))
    add("full-scatter-8x193", B=2, H=8, Hkv=2, Dh=128, Sq=8, Sk=193, mode="scatter", causal=False)
    add("full-pair-32x257", B=1, H=2, Hkv=1, Dh=64, Sq=32, Sk=257, mode="pair", pair=(63, 256), causal=False)
    return out


CASES = _cases()


def case_id(spec) -> str:
    return spec["name"]


def mutant_applies(case, mutant: str) -> bool:
    """Whether the construction is bound to see the fault at CHUNK = 64 (reasons, not measurements)."""
    s = case.spec
    Sq, Sk, G = s["Sq"], s["Sk"], s["H"] // s["Hkv"]
    nsplit = (Sk + CHUNK - 1) // CHUNK
    if mutant == "dropsplit":   # the last split holds the diagonal key of the last row
        return case.mode in ("diag", "negscale")
    if mutant == "norescale":   # every split then weighs in with its own best key (a pair over exactly two splits weighs 1 : 1 anyway)
        return nsplit > 2 or (nsplit == 2 and case.pair is None)
    if mutant == "edge+1":      # key 63 twice: the mean of the pair (63, 64) leans to 63
        return case.pair == (63, 64) or case.pair == (127, 128)
    if mutant == "edge-1":      # key 64 (128) never: the pair loses its second half
        return case.pair == (63, 64) or case.pair == (127, 128)
    if mutant == "mask+1":
        return case.mode == "decoy" and case.decoys > 0
    if mutant == "mask-1":
        return case.causal and case.mode in ("diag", "negscale")
    if mutant == "kvh+1":
        return s["Hkv"] > 1
    if mutant == "emptynan":    # causal, and the last split shorter than Sq - 1 keys: row 0 attends nothing of it
        return case.causal and Sq > 1 and Sk - (nsplit - 1) * CHUNK < Sq
    if mutant == "rowpack":     # the target depends on the row: a permutation of the rows shows
        return Sq > 1 and G > 1 and case.mode in ("diag", "negscale", "scatter")
    raise ValueError(mutant)
