"""Multi-LoRA on the adapted linears of Llama-3-8B, on the MI355X: the shrink + expand pair `ops.lora_apply` against the torch per-adapter
composition on the same tensors, beside the base `WQLinear` launch it follows.  Layers: qkv 4096 -> 6144 in three slices (4096 / 5120 / 6144),
o 4096 -> 4096, down 14336 -> 4096; bf16; pool rank 16 and 64; 64 slots.

Points per (layer, rank):
  decode, B = 1, 8, 64     one-token sequences, every sequence on its own adapter (the rectangular call)
  packed                   one step of 32 decodes plus a 512-token chunk, 33 adapters (cu_seqlens_q on the device)

Per point:
  pair / pair_graph        ops.lora_apply(x, y, ...) in place, eager / N calls captured into one graph and replayed   (+ a second measurement each)
  torch / torch_graph      per adapter: index_select of its rows, F.linear with A, F.linear with B, a scale, index_add_ into y.  The row indices
                           of every adapter are built BEFORE the clock starts, which flatters this path: a server would have to read the step's ids
                           on the host to build them, and that read is what keeps the real composition out of a graph.  The sliced qkv layer uses
                           ONE block-diagonal B [N, 3 R] so that the path keeps its two F.linear calls.
  base_graph               the base WQLinear (cdna4 layout) on the same x, captured

Method of tools/lm_head_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of its
measurements; the relative difference of two measurements of the same thing is the same-box noise; the margin of a point is the largest of that
noise and the spreads.  An eager figure is a host clock around N calls that end in a device synchronise; a graph figure is device events around
one replay of N captured calls.  The pools of a point (up to 170 MB) fit the 256 MB Infinity Cache: both paths may be flattered by hits a
serving loop never sees.

Goals (set before anything was measured):
  (a) at every decode point the pair is faster than the torch composition beyond the point's margin, graph against graph and eager against eager;
  (b) published without a goal: the pair's time over the base launch's (what a LoRA request pays), (A + B bytes of the named adapters) / time /
      8 TB/s, and the packed point.

The measurements run in a child process under a time limit.

  python tools/lora_bench.py [--out profiles/lora_bench.json] [--reps 5] [--ranks 16,64] [--layers qkv,o,down]
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

LAYERS = {"qkv": dict(K=4096, N=6144, slice_end=(4096, 5120, 6144)), "o": dict(K=4096, N=4096, slice_end=(4096,)),
          "down": dict(K=14336, N=4096, slice_end=(4096,))}
SLOTS = 64
HBM_BYTES_PER_S = 8e12
CHILD_TIMEOUT_S = 900
POINTS = (("decode", 1), ("decode", 8), ("decode", 64), ("packed", 33))


def point(torch, ops, layer, R, kind, B, base, a_pool, b_pool, scaling, reps, dev):
    from kvcache_attn_bench import graph_of, replay_us
    from lm_head_bench import eager_us
    import torch.nn.functional as F
    K, N, ends = LAYERS[layer]["K"], LAYERS[layer]["N"], LAYERS[layer]["slice_end"]
    ns = len(ends)
    gen = torch.Generator(device=dev).manual_seed(B + R)
    sq = [1] * B if kind == "decode" else [1] * 32 + [512]
    starts = [0]
    for s in sq:
        starts.append(starts[-1] + s)
    cu = None if kind == "decode" else torch.tensor(starts, dtype=torch.int32, device=dev)
    max_sq = max(sq)
    total_q = sum(sq)
    ids_host = list(range(B))                       # distinct adapters
    ids = torch.tensor(ids_host, dtype=torch.int32, device=dev)
    x = torch.randn(total_q, K, device=dev, generator=gen).to(torch.bfloat16)
    y0 = torch.randn(total_q, N, device=dev, generator=gen).to(torch.bfloat16)
    y_new, y_old = y0.clone(), y0.clone()
    ws = torch.empty(ops.lora_workspace_bytes(total_q, K, R, ns) // 4, dtype=torch.float32, device=dev)
    # the torch path's operands: per adapter its rows (built outside the clock), A [RS, K] and a block-diagonal B [N, RS]
    rows = [torch.arange(starts[b], starts[b + 1], device=dev) for b in range(B)]
    b_dense = []
    for a in ids_host:
        bd = torch.zeros(N, ns * R, dtype=torch.bfloat16, device=dev)
        lo = 0
        for j, hi in enumerate(ends):
            bd[lo:hi, j * R:(j + 1) * R] = b_pool[a, lo:hi]
            lo = hi
        b_dense.append(bd)
    scale_host = [float(s) for s in scaling.tolist()]
    n = 10 if B >= 33 else 20
    keep = []

    def new(y=y_new):
        return ops.lora_apply(x, y, a_pool, b_pool, scaling, ids, ends if ns > 1 else None, cu, max_sq, ws)

    def old(y=y_old):
        for b, a in enumerate(ids_host):
            xs = x.index_select(0, rows[b])
            d = F.linear(F.linear(xs, a_pool[a]), b_dense[b]) * scale_host[a]
            y.index_add_(0, rows[b], d)
        return y

    def base_call():
        return base(x)

    def many(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    # faster and different is not faster: one application of each path on the same y
    ya, yb = new(y0.clone()), old(y0.clone())
    diff = float((ya.float() - yb.float()).abs().max())
    eager = {"torch": old, "pair": new, "pair_again": new}
    graphs = {"torch_graph": graph_of(torch, many(old)), "pair_graph": graph_of(torch, many(new)), "pair_graph_again": graph_of(torch, many(new)),
              "base_graph": graph_of(torch, many(base_call))}
    for fn in eager.values():
        eager_us(torch, fn, 2)
    times = {name: [] for name in list(eager) + list(graphs)}
    for _ in range(reps):  # alternating
        for name, fn in eager.items():
            y_new.copy_(y0)
            y_old.copy_(y0)
            times[name].append(eager_us(torch, fn, n))
        for name, g in graphs.items():
            y_new.copy_(y0)
            y_old.copy_(y0)
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    adapter_bytes = len(set(ids_host)) * 2 * (ns * R * K + N * R)
    row = dict(layer=layer, K=K, N=N, slice_end=list(ends), rank=R, kind=kind, B=B, total_q=total_q, dtype="bfloat16", calls_per_measurement=n,
               plan=ops.lora_plan(K, R, ns), adapter_bytes=adapter_bytes, max_abs_difference_of_the_two_paths=diff)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise_eager"] = round(abs(best["pair"] - best["pair_again"]) / min(best["pair"], best["pair_again"]), 4)
    row["same_box_noise_graph"] = round(abs(best["pair_graph"] - best["pair_graph_again"]) / min(best["pair_graph"], best["pair_graph_again"]), 4)
    row["margin_eager"] = max(row["same_box_noise_eager"], row["torch_spread"], row["pair_spread"])
    row["margin_graph"] = max(row["same_box_noise_graph"], row["torch_graph_spread"], row["pair_graph_spread"])
    row["pair_over_torch_eager"] = round(best["pair"] / best["torch"], 4)
    row["pair_over_torch_graph"] = round(best["pair_graph"] / best["torch_graph"], 4)
    row["pair_over_base_graph"] = round(best["pair_graph"] / best["base_graph"], 4)
    row["pair_graph_fraction_of_8TBps"] = round(adapter_bytes / (best["pair_graph"] * 1e-6) / HBM_BYTES_PER_S, 4)
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    from llm_awq_amd import ops, synth
    from llm_awq_amd.qmodule import WQLinear

    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev = "cuda:0"
    with torch.no_grad():
        for layer in a.layers.split(","):
            K, N, ends = LAYERS[layer]["K"], LAYERS[layer]["N"], LAYERS[layer]["slice_end"]
            c = synth.random_wq(K, N, dtype=torch.bfloat16, device=dev, seed=K + N, keep_q=False)
            base = WQLinear(4, 128, K, N, False, dev, dtype=torch.bfloat16)
            base.load_state_dict(dict(qweight=c["qweight"], scales=c["scales"], scaled_zeros=c["scaled_zeros"]))
            base.to_cdna4()
            for R in [int(r) for r in a.ranks.split(",")]:
                gen = torch.Generator(device=dev).manual_seed(K + R)
                a_pool = torch.empty(SLOTS, len(ends) * R, K, dtype=torch.bfloat16, device=dev).normal_(0.0, K ** -0.5, generator=gen)
                b_pool = torch.empty(SLOTS, N, R, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02, generator=gen)
                scaling = torch.full((SLOTS,), 2.0, dtype=torch.float32, device=dev)
                for kind, B in POINTS:
                    print("ROW " + json.dumps(point(torch, ops, layer, R, kind, B, base, a_pool, b_pool, scaling, a.reps, dev)), flush=True)
                del a_pool, b_pool
                torch.cuda.empty_cache()


def verdicts(rows):
    """goal (a) per way of measuring, with the points that miss it named"""
    out = {}
    dec = [r for r in rows if r["kind"] == "decode"]
    for kind in ("eager", "graph"):
        miss = [f'{r["layer"]}/r{r["rank"]}/B{r["B"]}' for r in dec if not r["pair_over_torch_" + kind] < 1.0 - r["margin_" + kind]]
        out[f"{kind}/a_pair_faster_than_torch_at_every_decode_point"] = (not miss) if len(dec) == 18 else "not measured"
        out[f"{kind}/a_misses"] = miss
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--layers", default="qkv,o,down")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--ranks", a.ranks, "--layers", a.layers]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"lora_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"lora_bench: the measurements failed with exit status {r.returncode}; stopping")
    key = lambda r: f'{r["layer"]}/r{r["rank"]}/{r["kind"]}{r["B"]}'
    summary = dict(points=len(rows), goals=verdicts(rows),
                   pair_over_torch_graph={key(r): r["pair_over_torch_graph"] for r in rows},
                   pair_over_torch_eager={key(r): r["pair_over_torch_eager"] for r in rows},
                   pair_over_base_graph={key(r): r["pair_over_base_graph"] for r in rows},
                   pair_graph_us={key(r): r["pair_graph_us"] for r in rows},
                   pair_graph_fraction_of_8TBps={key(r): r["pair_graph_fraction_of_8TBps"] for r in rows},
                   not_measured=["fp16", "ranks other than 16 and 64", "hardware counters", "a whole model step", "a cold Infinity Cache"])
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shapes=LAYERS, slots=SLOTS, summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
