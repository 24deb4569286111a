"""Packed steps of continuous batching (attn_prefill_paged_varq, rope_kv_store_paged_varq) against the rectangular calls they replace, on the
MI355X.  Llama-3-8B's attention (H 32, Hkv 8, Dh 128), bf16, 256-key pages, shuffled tables.

  (a) uniform  4 x 512 new tokens over 2048 keys of history: ONE varq call against attn_prefill_paged on the same rectangle (the same kernel
               body and q tile: the same bits), and the varq store against rope_kv_store_paged_pos.  Prices the two scalar loads of
               cu_seqlens_q and the store's binary search.  Goal: no slower beyond the margin.
  (b) ragged   chunks of 37 / 200 / 512 / 1024 tokens over 0 / 512 / 2048 / 8192 keys: ONE call (max_seqlen_q = 1024) against the SUM of the
               four per-sequence attn_prefill_paged calls.  Goal: no slower beyond the margin.
  (c) mixed    32 one-token sequences at 2048 keys (and again at 32768) plus one 512-token chunk over 2048 keys: ONE varq call against
               attn_kvcache_paged for the 32 plus attn_prefill_paged for the chunk.  No goal: a one-token sequence inside a packed call runs
               the one-pass kernel, not the split pair; the figure tells a scheduler when to split its step.
  (d) loose    the batch of (b) under max_seqlen_q = 1024 against max_seqlen_q = 8192: the price of empty ranks.  No goal.

Method of tools/prefill_kvcache_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets replayed `reps` times; a
point reports the best replay and the spread of its replays; the two paths alternate in one process; the new form is captured twice, and the
relative difference of the two identical graphs is the same-box noise the ratio is read against.  A point is "slower beyond the margin" when
new / old > 1 + max(same-box noise, both spreads).

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/varq_prefill_bench.py [--out profiles/varq_prefill_bench.json] [--reps 5] [--only uniform,ragged,mixed,loose]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kvcache_attn_bench import DEV, DH, H, HKV, SCALE, time_pair  # noqa: E402

GROUPS = ("uniform", "ragged", "mixed", "loose")
CHILD_TIMEOUT_S = 420
PS = 256
SETS = 2
UNIFORM = [(512, 2048)] * 4                                   # (new tokens, history)
RAGGED = [(37, 0), (200, 512), (512, 2048), (1024, 8192)]
MIXED_HIST, MIXED_CHUNK = (2048, 32768), (512, 2048)
LOOSE_BOUNDS = (1024, 8192)
W = (H + 2 * HKV) * DH


def make_set(torch, seqs, seed, pad=0):
    """One packed step over a shuffled pool: q [T + pad, H, Dh], pools holding hist + new keys of every sequence, the table, cu_seqlens_q and
    the lengths before the step."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(seqs)
    totals = [s + h for s, h in seqs]
    need = [-(-n // PS) for n in totals]
    pps, P = max(need), sum(need)
    ids = torch.randperm(P, device=DEV, generator=g).int()
    table = torch.zeros(B, pps, dtype=torch.int32, device=DEV)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = ids[at:at + n]
        at += n
    kp = torch.randn(P, PS, HKV, DH, device=DEV, dtype=torch.bfloat16, generator=g)
    vp = 1 + 0.5 * torch.randn(P, PS, HKV, DH, device=DEV, dtype=torch.bfloat16, generator=g)
    T = sum(s for s, _ in seqs)
    q = (1.5 * torch.randn(T + pad, H, DH, device=DEV, generator=g)).to(torch.bfloat16)
    cu = torch.tensor([0] + [s for s, _ in seqs], dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)
    hist = torch.tensor([h for _, h in seqs], dtype=torch.int32, device=DEV)
    return dict(q=q, kp=kp, vp=vp, table=table, cu=cu, hist=hist, bound=pps * PS, seqs=seqs, cu_host=[0] + [int(x) for x in cu[1:].cpu()])


def varq_call(E, s, max_q):
    return E.attn_prefill_paged_varq(s["q"], s["kp"], s["vp"], s["table"], s["cu"], max_q, s["hist"], s["bound"], True, SCALE, True)


def alone(E, s, b):
    """Sequence b of a set through the rectangular one-pass entry: batch 1, its own table row and length."""
    lo, hi = s["cu_host"][b], s["cu_host"][b + 1]
    return E.attn_prefill_paged(s["q"][lo:hi].view(1, hi - lo, H, DH), s["kp"], s["vp"], s["table"][b:b + 1], s["hist"][b:b + 1], s["bound"],
                                hi - lo, SCALE, True)


def compare(torch, new, old, keep, n, reps, same=None, **row):
    new()
    got = [t.clone() for t in keep]
    old()
    if same is not None:
        row["same_bits"] = same(got, keep)
    row.update(time_pair(torch, new, old, n, reps))
    return row


def uniform_points(torch, E, ops, reps, emit):
    sets = [make_set(torch, UNIFORM, i) for i in range(SETS)]
    B, S = len(UNIFORM), UNIFORM[0][0]
    keep = []

    def new():
        keep.clear()
        for s in sets:
            keep.append(varq_call(E, s, S))

    def old():
        keep.clear()
        for s in sets:
            keep.append(E.attn_prefill_paged(s["q"].view(B, S, H, DH), s["kp"], s["vp"], s["table"], s["hist"], s["bound"], S, SCALE, True).view(B * S, H, DH))
    emit(compare(torch, new, old, keep, SETS, reps, same=lambda a, b: all(bool(torch.equal(x.view(torch.int16), y.view(torch.int16))) for x, y in zip(a, b)),
                 point="uniform-attn", goal="a", seqs=UNIFORM, q_tile=ops.attn_varq_plan(B, H, HKV, DH, S)[0],
                 q_tile_rect=ops.attn_prefill_plan(B, H, HKV, DH, S, sets[0]["bound"])[0]))
    # the store: the same tokens into pools of their own
    freqs = torch.randn(sets[0]["bound"], DH, device=DEV)
    xs = [torch.randn(B * S, W, device=DEV).to(torch.bfloat16) for _ in sets]
    mine = [(torch.zeros_like(s["kp"]), torch.zeros_like(s["vp"])) for s in sets]
    theirs = [(torch.zeros_like(s["kp"]), torch.zeros_like(s["vp"])) for s in sets]

    def new_store():
        keep.clear()
        for s, x, (kp, vp) in zip(sets, xs, mine):
            keep.append(E.rope_kv_store_paged_varq(x, freqs, kp, vp, s["table"], s["cu"], S, s["hist"], H, HKV))

    def old_store():
        keep.clear()
        for s, x, (kp, vp) in zip(sets, xs, theirs):
            keep.append(E.rope_kv_store_paged_pos(x.view(B, S, W), freqs, kp, vp, s["table"], s["hist"], H, HKV).view(B * S, H, DH))
    row = compare(torch, new_store, old_store, keep, SETS, reps,
                  same=lambda a, b: all(bool(torch.equal(x.view(torch.int16), y.view(torch.int16))) for x, y in zip(a, b)),
                  point="uniform-store", goal="a", seqs=UNIFORM)
    row["same_pools"] = all(bool(torch.equal(a.view(torch.int16), b.view(torch.int16))) for m, t in zip(mine, theirs) for a, b in zip(m, t))
    emit(row)


def ragged_points(torch, E, ops, reps, emit, bounds=(1024,), goal="b"):
    sets = [make_set(torch, RAGGED, 10 + i) for i in range(SETS)]
    keep = []

    def rows_same(a, b):
        return all(bool(torch.equal(x.view(torch.int16), y.view(torch.int16))) for x, y in zip(a, b))
    if goal == "b":
        def new():
            keep.clear()
            for s in sets:
                keep.append(varq_call(E, s, bounds[0]))

        def old():   # the sum of the four per-sequence calls
            keep.clear()
            for s in sets:
                keep.append(torch.cat([alone(E, s, b)[0] for b in range(len(RAGGED))], 0))
        # (the plan takes B and Sq: a single short chunk may run another q tile, so equal bits are reported, not required)
        emit(compare(torch, new, old, keep, SETS, reps, same=rows_same, point="ragged", goal="b", seqs=RAGGED, max_seqlen_q=bounds[0],
                     q_tile=ops.attn_varq_plan(len(RAGGED), H, HKV, DH, bounds[0])[0],
                     q_tile_single=[ops.attn_prefill_plan(1, H, HKV, DH, s, s + h)[0] for s, h in RAGGED]))
        return
    tight, loose = bounds

    def new():
        keep.clear()
        for s in sets:
            keep.append(varq_call(E, s, loose))

    def old():
        keep.clear()
        for s in sets:
            keep.append(varq_call(E, s, tight))
    emit(compare(torch, new, old, keep, SETS, reps, same=rows_same, point="loose", goal="d", seqs=RAGGED, max_seqlen_q_new=loose, max_seqlen_q_old=tight,
                 blocks_new=ops.attn_varq_plan(len(RAGGED), H, HKV, DH, loose)[1], blocks_old=ops.attn_varq_plan(len(RAGGED), H, HKV, DH, tight)[1]))


def mixed_points(torch, E, ops, reps, emit):
    for hist in MIXED_HIST:
        seqs = [(1, hist)] * 32 + [MIXED_CHUNK]
        sets = [make_set(torch, seqs, 20 + i) for i in range(SETS)]
        keep = []

        def new():
            keep.clear()
            for s in sets:
                keep.append(varq_call(E, s, MIXED_CHUNK[0]))

        def old():   # the split pair for the 32 decodes, the one-pass kernel for the chunk
            keep.clear()
            for s in sets:
                dec = E.attn_kvcache_paged(s["q"][:32].view(32, 1, H, DH), s["kp"], s["vp"], s["table"][:32], s["hist"][:32], s["bound"], 1, SCALE, True)
                keep.append(torch.cat([dec.view(32, H, DH), alone(E, s, 32)[0]], 0))
        new()
        got = [t.clone() for t in keep]
        old()
        diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(got, keep))
        row = dict(point="mixed", goal="c", decodes=32, decode_history=hist, chunk=list(MIXED_CHUNK), max_abs_diff_of_outputs=round(diff, 6))
        row.update(time_pair(torch, new, old, SETS, reps))   # (one pass against the split pair: the same mathematics, not the same bits)
        emit(row)
        del sets
        torch.cuda.empty_cache()


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("varq_prefill_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)
    if a.group == "uniform":
        uniform_points(torch, E, ops, a.reps, emit)
    elif a.group == "ragged":
        ragged_points(torch, E, ops, a.reps, emit)
    elif a.group == "loose":
        ragged_points(torch, E, ops, a.reps, emit, bounds=LOOSE_BOUNDS, goal="d")
    else:
        mixed_points(torch, E, ops, a.reps, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varq_prefill_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="uniform", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"varq_prefill_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"varq_prefill_bench: {group} failed with exit status {r.returncode}; stopping")

    def margin(r):
        return max(r["same_box_noise"], r["new_spread"], r["old_spread"])

    def verdict(goal):
        mine = [r for r in rows if r["goal"] == goal]
        return dict(ratios={r["point"]: r["new_over_old"] for r in mine}, margins={r["point"]: round(margin(r), 4) for r in mine},
                    misses=[[r["point"], r["new_over_old"], round(margin(r), 4)] for r in mine if r["new_over_old"] > 1.0 + margin(r)])
    summary = dict(points=len(rows), groups=a.only, a_uniform_no_slower_than_the_rectangle=verdict("a"),
                   b_ragged_no_slower_than_the_sum=verdict("b"),
                   c_mixed_step_published_without_a_goal={str(r["decode_history"]): r["new_over_old"] for r in rows if r["goal"] == "c"},
                   d_loose_bound_published_without_a_goal={r["point"]: r["new_over_old"] for r in rows if r["goal"] == "d"})
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, dtype="bfloat16", page_size=PS), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
