"""Routing of many-expert models on the MI355X: ops.moe_route_scored against the torch glue with the same router (MoeRouter.route_torch +
moe.sort_by_expert -- what SparseMoeMLP(routing="torch", router=...) runs, and the only way these shapes were served before the entry existed).
fp32 logits, routing only (no expert matmul).

Points:
  qwen3   E 128, k 8, softmax, renormalised                                         T = 1, 64, 4096
  dsv3    E 256, k 8, sigmoid + bias, 8 groups of which 4, group score top-2, x 2.5  T = 1, 64, 4096
  e64     E 64,  k 8, softmax: against the existing ops.moe_route, for information   T = 64, 4096

Per point:
  old_eager        the torch glue (or ops.moe_route for e64), eager: it cannot be captured (torch.bincount reads back to the host)
  new_eager        ops.moe_route_scored, eager                 (+ a second measurement of the same thing)
  new_graph        the same captured into one hipGraph of N calls and replayed (for e64 also old_graph)

Method of tools/moe_route_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of
its measurements, and the relative difference of two measurements of the same thing is the same-box noise a ratio is read against.  An eager
figure is a host clock around N calls that end in a device synchronise; a graph figure is device events around one replay of N captured calls.

Goal (set before anything was measured): at every qwen3 / dsv3 point moe_route_scored is faster than the torch glue beyond the margin (the
largest of the same-box noise and the two spreads), eager against eager.

The measurements run in a child process under a time limit.

  python tools/moe_route_scored_bench.py [--out profiles/moe_route_scored_bench.json] [--reps 5]
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

CHILD_TIMEOUT_S = 420
POINTS = [("qwen3", 128, 8, (1, 64, 4096)), ("dsv3", 256, 8, (1, 64, 4096)), ("e64", 64, 8, (64, 4096))]


def point(torch, name, E, k, T, reps, dev):
    from kvcache_attn_bench import graph_of, replay_us
    from moe_route_bench import eager_us

    from llm_awq_amd import moe as MOE
    from llm_awq_amd import ops
    gen = torch.Generator(device=dev).manual_seed(T + E)
    logits = torch.randn(T, E, device=dev, generator=gen)
    if name == "dsv3":
        bias = (torch.rand(E, device=dev, generator=gen) - 0.5).contiguous()
        router = MOE.MoeRouter("sigmoid", True, bias, n_group=8, topk_group=4, group_top=2, scale=2.5)
    else:
        router = MOE.MoeRouter()
    kw = router.kwargs()

    def new():
        return ops.moe_route_scored(logits, k, **kw)

    def old():
        if name == "e64":
            return ops.moe_route(logits, k)
        ids, w = router.route_torch(logits, k)
        return (ids, w) + MOE.sort_by_expert(ids, E)
    n = 200 if T <= 64 else 50
    keep = []

    def n_calls(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    a, b = new(), old()
    same_ids = float((a[0].long() == b[0].long()).float().mean())   # (fp32 against fp32 keys: near ties may differ)
    eager = {"old_eager": old, "new_eager": new, "new_eager_again": new}
    graphs = {"new_graph": graph_of(torch, n_calls(new))}
    if name == "e64":
        graphs["old_graph"] = graph_of(torch, n_calls(old))
    for fn in eager.values():  # warm-up
        eager_us(torch, fn, 3)
    times = {nm: [] for nm in list(eager) + list(graphs)}
    for _ in range(reps):  # alternating
        for nm, fn in eager.items():
            times[nm].append(eager_us(torch, fn, n))
        for nm, g in graphs.items():
            times[nm].append(replay_us(torch, g) / n)
    best = {nm: min(t) for nm, t in times.items()}
    row = dict(point=name, experts=E, top_k=k, tokens=T, calls_per_measurement=n, ids_equal_fraction=round(same_ids, 6))
    for nm, t in times.items():
        row[nm + "_us"] = round(best[nm], 2)
        row[nm + "_spread"] = round((max(t) - best[nm]) / best[nm], 4)
    row["same_box_noise_eager"] = round(abs(best["new_eager"] - best["new_eager_again"]) / min(best["new_eager"], best["new_eager_again"]), 4)
    row["new_over_old_eager"] = round(best["new_eager"] / best["old_eager"], 4)
    row["margin_eager"] = max(row["same_box_noise_eager"], row["old_eager_spread"], row["new_eager_spread"])
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("moe_route_scored_bench needs the GPU: there is no CPU timing of a GPU kernel")
    with torch.no_grad():
        for name, E, k, tokens in POINTS:
            for T in tokens:
                print("ROW " + json.dumps(point(torch, name, E, k, T, a.reps, "cuda:0")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_route_scored_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"moe_route_scored_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"moe_route_scored_bench: the measurements failed with exit status {r.returncode}; stopping")
    goal = [r for r in rows if r["point"] != "e64"]
    summary = dict(points=len(rows),
                   goal_faster_than_torch_glue_beyond_margin=(all(r["new_over_old_eager"] < 1.0 - r["margin_eager"] for r in goal) if goal else "not measured"),
                   new_over_old_eager={f'{r["point"]}/{r["tokens"]}': r["new_over_old_eager"] for r in rows},
                   margin_eager={f'{r["point"]}/{r["tokens"]}': r["margin_eager"] for r in rows})
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(logits="float32", summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
