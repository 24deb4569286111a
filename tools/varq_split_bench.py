"""A mixed packed step (attn_paged_varq: the split-KV pair for the short sequences, the one-pass kernel for the rest) against the two ways
of running the same step today, on the MI355X.  Llama-3-8B's attention (H 32, Hkv 8, Dh 128), bf16, 256-key pages, shuffled tables,
split_seqlen_q = 1, the default floor (ops.ATTN_SPLIT_MIN_KEYS) unless a point says otherwise.

  (1) mixed   32 one-token sequences at 2048 keys (and again at 32768) plus one 512-token chunk over 2048 keys: attn_paged_varq against
              attn_prefill_paged_varq on the same step, and against the rectangular pair attn_kvcache_paged + attn_prefill_paged.
              Goals: faster than attn_prefill_paged_varq beyond the margin at both key counts; no slower than the pair beyond the margin.
  (2) prompt  the pure prompt batch (b) of tools/varq_prefill_bench.py -- no sequence is taken: attn_paged_varq against
              attn_prefill_paged_varq.  The price of two launches of empty blocks.  No goal.
  (3) floor   one (and 32) one-token sequences at 512 / 1024 / 2048 / 4096 keys next to the 512-token chunk: split_min_keys = 64 (the pair
              serves them) against a floor above the length (the one-pass kernel serves them).  Shows where the floor belongs.  No goal.

Method of tools/varq_prefill_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets; the paths of a point
alternate in one process; a figure is the best of `reps` replays with the spread of its replays; the first path is captured twice and the
relative difference of the two identical graphs is the same-box noise.  margin = max(same-box noise, the spreads of the two paths compared).

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/varq_split_bench.py [--out profiles/varq_split_bench.json] [--reps 5] [--only mixed,prompt,floor]
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

from kvcache_attn_bench import DH, H, HKV, SCALE, graph_of, replay_us  # noqa: E402
from varq_prefill_bench import MIXED_CHUNK, MIXED_HIST, PS, RAGGED, SETS, alone, make_set, varq_call  # noqa: E402

GROUPS = ("mixed", "prompt", "floor")
CHILD_TIMEOUT_S = 420
FLOOR_KEYS = (512, 1024, 2048, 4096)
FLOOR_DECODES = (1, 32)


def time_paths(torch, paths, n, reps):
    """paths: {name: function that issues the N calls of one graph}; the first path is captured a second time for the same-box noise."""
    first = next(iter(paths))
    graphs = {name: graph_of(torch, fn) for name, fn in paths.items()}
    graphs[first + "_again"] = graph_of(torch, paths[first])
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(calls_per_graph=n)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise"] = round(abs(best[first] - best[first + "_again"]) / min(best[first], best[first + "_again"]), 4)
    del graphs
    return row, best


def against(row, best, new, old):
    """new / old and the margin it is read against."""
    ratio = round(best[new] / best[old], 4)
    margin = round(max(row["same_box_noise"], row[new + "_spread"], row[old + "_spread"]), 4)
    verdict = "faster" if ratio < 1.0 - margin else ("slower" if ratio > 1.0 + margin else "within the margin")
    return dict(ratio=ratio, margin=margin, verdict=verdict)


def mix_call(E, s, max_q, floor, split_q=1):
    return E.attn_paged_varq(s["q"], s["kp"], s["vp"], s["table"], s["cu"], max_q, s["hist"], s["bound"], split_q, floor, True, SCALE, True)


def rect_pair(torch, E, s, n):
    """The n one-token sequences by the rectangular split pair, the chunk behind them by the rectangular one-pass kernel."""
    dec = E.attn_kvcache_paged(s["q"][:n].view(n, 1, H, DH), s["kp"], s["vp"], s["table"][:n], s["hist"][:n], s["bound"], 1, SCALE, True)
    return torch.cat([dec.view(n, H, DH), alone(E, s, n)[0]], 0)


def same_bits(torch, a, b):
    return all(bool(torch.equal(x.view(torch.int16), y.view(torch.int16))) for x, y in zip(a, b))


def run_paths(torch, paths, sets):
    """One eager pass of every path: {name: the outputs of the sets}."""
    return {name: [fn(s).clone() for s in sets] for name, fn in paths.items()}


def graph_fns(paths, sets, keep):
    def of(fn):
        def go():
            keep.clear()
            for s in sets:
                keep.append(fn(s))
        return go
    return {name: of(fn) for name, fn in paths.items()}


def mixed_points(torch, E, ops, reps, emit):
    floor, maxq = ops.ATTN_SPLIT_MIN_KEYS, MIXED_CHUNK[0]
    for hist in MIXED_HIST:
        seqs = [(1, hist)] * 32 + [MIXED_CHUNK]
        sets = [make_set(torch, seqs, 20 + i) for i in range(SETS)]
        paths = dict(varq_split=lambda s: mix_call(E, s, maxq, floor), varq_one_pass=lambda s: varq_call(E, s, maxq),
                     rect_pair=lambda s: rect_pair(torch, E, s, 32))
        outs = run_paths(torch, paths, sets)
        keep = []
        row, best = time_paths(torch, graph_fns(paths, sets, keep), SETS, reps)
        row.update(point="mixed", decodes=32, decode_history=hist, chunk=list(MIXED_CHUNK), split_min_keys=floor,
                   split_plan=list(ops.attn_varq_split_plan(33, H, HKV, DH, 1, sets[0]["bound"])),
                   same_bits_as_rect_pair=same_bits(torch, outs["varq_split"], outs["rect_pair"]),
                   chunk_rows_same_bits_as_one_pass=same_bits(torch, [o[32:] for o in outs["varq_split"]], [o[32:] for o in outs["varq_one_pass"]]),
                   vs_one_pass=against(row, best, "varq_split", "varq_one_pass"), vs_rect_pair=against(row, best, "varq_split", "rect_pair"))
        emit(row)
        del sets, outs
        torch.cuda.empty_cache()


def prompt_points(torch, E, ops, reps, emit):
    maxq = 1024
    sets = [make_set(torch, RAGGED, 10 + i) for i in range(SETS)]
    paths = dict(varq_split=lambda s: mix_call(E, s, maxq, ops.ATTN_SPLIT_MIN_KEYS), varq_one_pass=lambda s: varq_call(E, s, maxq))
    outs = run_paths(torch, paths, sets)
    keep = []
    row, best = time_paths(torch, graph_fns(paths, sets, keep), SETS, reps)
    row.update(point="prompt", seqs=RAGGED, max_seqlen_q=maxq, split_min_keys=ops.ATTN_SPLIT_MIN_KEYS,
               split_plan=list(ops.attn_varq_split_plan(len(RAGGED), H, HKV, DH, 1, sets[0]["bound"])),
               same_bits=same_bits(torch, outs["varq_split"], outs["varq_one_pass"]), vs_one_pass=against(row, best, "varq_split", "varq_one_pass"))
    emit(row)


def floor_points(torch, E, ops, reps, emit):
    maxq = MIXED_CHUNK[0]
    for n in FLOOR_DECODES:
        for keys in FLOOR_KEYS:
            seqs = [(1, keys - 1)] * n + [MIXED_CHUNK]          # Sk_b = keys
            sets = [make_set(torch, seqs, 30 + i) for i in range(SETS)]
            paths = dict(floor_64=lambda s: mix_call(E, s, maxq, 64), floor_above=lambda s: mix_call(E, s, maxq, keys + 1))
            keep = []
            row, best = time_paths(torch, graph_fns(paths, sets, keep), SETS, reps)
            row.update(point="floor", decodes=n, decode_keys=keys, chunk=list(MIXED_CHUNK),
                       split_plan=list(ops.attn_varq_split_plan(n + 1, H, HKV, DH, 1, sets[0]["bound"])),
                       split_vs_one_pass=against(row, best, "floor_64", "floor_above"))
            emit(row)
            del sets
            torch.cuda.empty_cache()


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("varq_split_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)
    {"mixed": mixed_points, "prompt": prompt_points, "floor": floor_points}[a.group](torch, E, ops, a.reps, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varq_split_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="mixed", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"varq_split_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"varq_split_bench: {group} failed with exit status {r.returncode}; stopping")
    mixed = [r for r in rows if r["point"] == "mixed"]
    summary = dict(
        points=len(rows), groups=a.only,
        goal_1a_faster_than_the_one_pass_step={str(r["decode_history"]): r["vs_one_pass"] for r in mixed},
        goal_1a_met=bool(mixed) and all(r["vs_one_pass"]["verdict"] == "faster" for r in mixed),
        goal_1b_no_slower_than_the_rectangular_pair={str(r["decode_history"]): r["vs_rect_pair"] for r in mixed},
        goal_1b_met=bool(mixed) and all(r["vs_rect_pair"]["verdict"] != "slower" for r in mixed),
        prompt_batch_published_without_a_goal={r["point"]: r["vs_one_pass"] for r in rows if r["point"] == "prompt"},
        floor_published_without_a_goal={f"{r['decodes']}x1@{r['decode_keys']}": r["split_vs_one_pass"] for r in rows if r["point"] == "floor"})
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, dtype="bfloat16", page_size=PS, split_seqlen_q=1), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
