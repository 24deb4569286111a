"""The Mixtral expert block with its routing, on the MI355X: SparseMoeMLP(routing="torch") against SparseMoeMLP(routing="device").
Mixtral-8x7B shapes (E 8, top-2, H 4096, F 14336), W4A16 g128, bf16, the fused gate/up module; T = 1, 4, 8, 64, 256, 2048 tokens.

Per point:
  torch_eager      the whole block with the torch routing glue, eager (it cannot be captured: torch.bincount reads back to the host)
  device_eager     the whole block with the three routing launches, eager          (+ a second measurement of the same thing)
  device_graph     the same captured into one hipGraph of N forwards and replayed  (+ a second graph of the same thing)
  routing_graph    moe_route + moe_gather + moe_combine on their own (no expert matmul), captured

Method of tools/paged_attn_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of
its measurements, and the relative difference of two measurements of the same thing is the same-box noise a ratio is read against.  An eager
figure is a host clock around N calls that end in a device synchronise; a graph figure is device events around one replay of N captured calls.

Goals (set before anything was measured): routing="device" is faster than routing="torch" beyond noise at every T <= 8 (eager against eager),
and not slower beyond noise at T = 2048.

The measurements run in a child process under a time limit.

  python tools/moe_route_bench.py [--out profiles/moe_route_bench.json] [--reps 5] [--tokens 1,4,8,64,256,2048]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

E, TOP_K, H, F = 8, 2, 4096, 14336
CHILD_TIMEOUT_S = 540


def build_blocks(torch, dev, dtype):
    """(routing='torch' block, routing='device' block) over the same random Mixtral-sized experts (timing only: the weights are random codes with
    scales of a N(0, 0.02^2) layer, as bench_extra.moe_mixtral draws them)"""
    from llm_awq_amd import moe as MOE
    from llm_awq_amd import ops
    from llm_awq_amd.qmodule import WQLinear
    gen = torch.Generator(device=dev).manual_seed(505)

    def rand_lin(K, N):
        m = WQLinear(4, 128, K, N, False, dev, dtype=dtype)
        m.qweight = ops.pack_v2(torch.randint(0, 16, (N, K), dtype=torch.uint8, device=dev, generator=gen))
        G = K // 128
        s, z = torch.zeros_like(m.scales), torch.zeros_like(m.scaled_zeros)
        s[:G] = ((5.2 + 0.8 * torch.rand(G, N, device=dev, generator=gen)) * 0.02 / 15).to(dtype)
        z[:G] = -(s[:G].float() * torch.randint(5, 11, (G, N), device=dev, generator=gen).float()).to(dtype)
        m.scales, m.scaled_zeros = s, z
        return m
    w1, w3, w2 = [rand_lin(H, F) for _ in range(E)], [rand_lin(H, F) for _ in range(E)], [rand_lin(F, H) for _ in range(E)]
    g2 = MOE.GroupedWQLinear(w2).to_cdna4()
    tor = MOE.SparseMoeMLP.fused(w1, w3, g2, TOP_K)
    del w1, w3, w2
    return tor, MOE.SparseMoeMLP(None, None, g2, TOP_K, tor.gate_up, routing="device")


def eager_us(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def point(torch, ops, tor, dev_blk, T, reps, dev, dtype):
    from kvcache_attn_bench import graph_of, replay_us
    gen = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(T, H, device=dev, generator=gen).to(dtype)
    logits = torch.randn(T, E, device=dev, generator=gen)
    n = 100 if T <= 64 else (40 if T <= 256 else 16)
    keep = []
    y_t, y_d = tor(x, logits), dev_blk(x, logits)
    rel = float((y_d.float() - y_t.float()).norm() / y_t.float().norm())
    _ids, w, order, inv, _off = ops.moe_route(logits, TOP_K)
    ys = torch.randn(T * TOP_K, H, device=dev, generator=gen).to(dtype)

    def n_device():
        keep.clear()
        for _ in range(n):
            keep.append(dev_blk(x, logits))

    def n_routing():
        keep.clear()
        for _ in range(n):
            r = ops.moe_route(logits, TOP_K)
            keep.append((ops.moe_gather(x, r[2], TOP_K), ops.moe_combine(ys, r[3], r[1])))
    graphs = {"device_graph": graph_of(torch, n_device), "device_graph_again": graph_of(torch, n_device), "routing_graph": graph_of(torch, n_routing)}
    eager = {"torch_eager": lambda: tor(x, logits), "device_eager": lambda: dev_blk(x, logits), "device_eager_again": lambda: dev_blk(x, logits)}
    for fn in eager.values():  # warm-up
        eager_us(torch, fn, 3)
    times = {name: [] for name in list(eager) + list(graphs)}
    for _ in range(reps):  # alternating
        for name, fn in eager.items():
            times[name].append(eager_us(torch, fn, n))
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(point="block", tokens=T, calls_per_measurement=n, rel_diff_device_vs_torch=round(rel, 6))
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)

    def noise(a, b):
        return round(abs(best[a] - best[b]) / min(best[a], best[b]), 4)
    row["same_box_noise_eager"] = noise("device_eager", "device_eager_again")
    row["same_box_noise_graph"] = noise("device_graph", "device_graph_again")
    row["device_over_torch_eager"] = round(best["device_eager"] / best["torch_eager"], 4)
    row["device_graph_over_torch_eager"] = round(best["device_graph"] / best["torch_eager"], 4)
    row["margin_eager"] = max(row["same_box_noise_eager"], row["torch_eager_spread"], row["device_eager_spread"])
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("moe_route_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev, dtype = "cuda:0", torch.bfloat16
    torch.manual_seed(0)
    with torch.no_grad():
        tor, dev_blk = build_blocks(torch, dev, dtype)
        for T in [int(t) for t in a.tokens.split(",")]:
            print("ROW " + json.dumps(point(torch, ops, tor, dev_blk, T, a.reps, dev, dtype)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_route_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", default="1,4,8,64,256,2048")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--tokens", a.tokens]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"moe_route_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"moe_route_bench: the measurements failed with exit status {r.returncode}; stopping")
    decode = [r for r in rows if r["tokens"] <= 8]
    big = [r for r in rows if r["tokens"] == 2048]
    summary = dict(points=len(rows),
                   goal_faster_beyond_noise_at_T_le_8=(all(r["device_over_torch_eager"] < 1.0 - r["margin_eager"] for r in decode) if decode else "not measured"),
                   goal_not_slower_beyond_noise_at_2048=(all(r["device_over_torch_eager"] <= 1.0 + r["margin_eager"] for r in big) if big else "not measured"),
                   device_over_torch_eager={r["tokens"]: r["device_over_torch_eager"] for r in rows},
                   device_graph_over_torch_eager={r["tokens"]: r["device_graph_over_torch_eager"] for r in rows},
                   margin_eager={r["tokens"]: r["margin_eager"] for r in rows})
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(E=E, top_k=TOP_K, H=H, F=F, dtype="bfloat16", weights="W4A16 g128, fused gate/up"), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
