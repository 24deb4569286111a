"""AWQ quantisation on the MI355X: the three launches of llm_awq_amd.quantize against the torch compositions they replace, on the Llama-3-8B
linears (N x K = 4096 x 4096, 14336 x 4096, 4096 x 14336), bf16, 512 tokens.

Per shape:
  clip_search      ops.clip_search(w, x)                        against  the reference's auto_clip_layer loop written with torch on the same GPU tensors
                                                                          (256 output channels at a time, ten shrink steps, sums in T)
  quantize_linear  WQLinear.quantize_linear(linear) (one launch +      against  torch fake-quantisation + WQLinear.from_linear + .to_cdna4()
                   the side buffers); the bare ops.quantize_pack launch is timed beside it
  fake_quant       quantize.fake_quant_scaled(w, s)             against  torch's pseudo-quantisation of w * s, divided by s

Method of tools/lm_head_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of its
measurements, the new path is measured twice and the relative difference of the two is the same-box noise; the margin of a comparison is the
largest of that noise and the two spreads.  A figure is a host clock around `calls` calls that end in a device synchronise; at 0.03 ... 0.2 ms
that holds launch and Python overhead as much as kernel time, so the two short launches (fake_quant on both paths, the bare quantize_pack) are
measured again as device time: ten captured calls, device events around one replay (`*_graph_ms`).  quantize_linear and its torch route read
a flag back from the device and cannot be captured.

Goals (set before anything was measured): each new path is faster than its torch composition beyond the margin at every shape.  Published
without a goal: clip_search's fraction of 2.5 PFLOP/s, 2 * 11 * N * K * S / time.  Besides the times a row records whether the two paths of a
comparison agree: bit equality for the two quantisers, the fraction of cells with the same clip index for the search (the torch loop sums in
bf16, the kernel in fp32).

The measurements run in a child process under a time limit.

  python tools/awq_quant_bench.py [--out profiles/awq_quant_bench.json] [--reps 5] [--shapes 4096x4096,14336x4096,4096x14336] [--tokens 512]
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

N_GRID, N_STEPS, N_BIT = 20, 10, 4
PEAK_FLOPS = 2.5e15
CHILD_TIMEOUT_S = 900
GRAPH_CALLS = 10


def torch_fake(torch, w, n_bit=N_BIT):
    """the grid of pseudo_quantize_tensor(zero_point=True, q_group_size=128) with torch operations -> (fake, scales, zeros)"""
    g = w.reshape(-1, 128)
    hi, lo, qmax = g.amax(dim=1, keepdim=True), g.amin(dim=1, keepdim=True), 2 ** n_bit - 1
    s = (hi - lo).clamp(min=1e-5) / qmax
    z = (-torch.round(lo / s)).clamp_(0, qmax)
    fake = (torch.clamp(torch.round(g / s) + z, 0, qmax) - z) * s
    return fake.reshape(w.shape), s.view(w.shape[0], -1), z.view(w.shape[0], -1)


def torch_clip(torch, w, x, rows=256):
    """auto_clip_layer's search with torch broadcasts: [rows, tokens, groups, 128] products per shrink step, summed in T -> (best [N, G], index)"""
    N, K = w.shape
    G = K // 128
    xg = x.reshape(1, x.shape[0], G, 128)
    best_all, idx_all = [], []
    for r0 in range(0, N, rows):
        wg = w[r0:r0 + rows].reshape(-1, 1, G, 128)
        m = wg.abs().amax(dim=-1, keepdim=True)
        best, low = m.clone(), torch.full_like(m, 1e9)
        idx = torch.zeros_like(m, dtype=torch.int32)
        ref = (xg * wg).sum(dim=-1)
        for i in range(N_STEPS):
            mv = m * (1 - i / N_GRID)
            q = torch_fake(torch, torch.clamp(wg, -mv, mv))[0]
            e = ((xg * q).sum(dim=-1) - ref).pow(2).mean(dim=1).view(low.shape)
            take = e < low
            low[take], best[take] = e[take], mv[take]
            idx[take] = i
        best_all.append(best)
        idx_all.append(idx)
    return torch.cat(best_all).reshape(N, G), torch.cat(idx_all).reshape(N, G)


def eager_ms(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def compare(torch, paths, reps, calls):
    """paths: {"torch": fn, "new": fn, ...}; "new" is measured twice.  -> dict of best times, spreads, noise, margin, ratio"""
    order = dict(paths)
    order["new_again"] = paths["new"]
    for name, fn in order.items():
        eager_ms(torch, fn, 1)  # warm-up
    times = {name: [] for name in order}
    for _ in range(reps):
        for name, fn in order.items():
            times[name].append(eager_ms(torch, fn, calls[name] if name in calls else calls["new"]))
    best = {name: min(t) for name, t in times.items()}
    out = {}
    for name, t in times.items():
        out[name + "_ms"] = round(best[name], 4)
        out[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    out["same_box_noise"] = round(abs(best["new"] - best["new_again"]) / min(best["new"], best["new_again"]), 4)
    out["margin"] = max(out["same_box_noise"], out["torch_spread"], out["new_spread"])
    out["new_over_torch"] = round(best["new"] / best["torch"], 5)
    out["faster_beyond_margin"] = bool(best["new"] * (1.0 + out["margin"]) < best["torch"])
    return out


def graph_figures(torch, paths, reps):
    from kvcache_attn_bench import graph_of, replay_us

    keep = []

    def many(fn):
        def run():
            keep.clear()
            for _ in range(GRAPH_CALLS):
                keep.append(fn())
        return run
    graphs = {name: graph_of(torch, many(fn)) for name, fn in paths.items()}
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / GRAPH_CALLS * 1e-3)
    best = {name: min(t) for name, t in times.items()}
    out = {}
    for name, t in times.items():
        out[name + "_graph_ms"] = round(best[name], 4)
        out[name + "_graph_spread"] = round((max(t) - best[name]) / best[name], 4)
    noise = abs(best["fake_quant_new"] - best["fake_quant_new_again"]) / min(best["fake_quant_new"], best["fake_quant_new_again"])
    out["fake_quant_graph_same_box_noise"] = round(noise, 4)
    out["fake_quant_graph_margin"] = max(out["fake_quant_graph_same_box_noise"], out["fake_quant_torch_graph_spread"], out["fake_quant_new_graph_spread"])
    out["fake_quant_graph_new_over_torch"] = round(best["fake_quant_new"] / best["fake_quant_torch"], 5)
    out["fake_quant_graph_faster_beyond_margin"] = bool(best["fake_quant_new"] * (1.0 + out["fake_quant_graph_margin"]) < best["fake_quant_torch"])
    del graphs, keep
    return out


def point(torch, N, K, S, reps, dev):
    from llm_awq_amd import ops, quantize
    from llm_awq_amd.qmodule import WQLinear

    gen = torch.Generator(device=dev).manual_seed(N + K)
    w = torch.empty(N, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02, generator=gen)
    x = torch.randn(S, K, device=dev, generator=gen).to(torch.bfloat16)
    cs = (0.25 + 3.75 * torch.rand(K, device=dev, generator=gen)).to(torch.bfloat16)
    lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device=dev)
    lin.weight.data = w
    row = dict(N=N, K=K, S=S, dtype="bfloat16", n_bit=N_BIT, n_grid=N_GRID, n_steps=N_STEPS)

    # clip search
    best_new, idx_new = ops.clip_search(w, x, N_BIT, N_GRID, N_STEPS)
    best_old, idx_old = torch_clip(torch, w, x)
    row["clip_same_index_fraction"] = round(float((idx_new == idx_old).float().mean()), 4)
    c = compare(torch, {"torch": lambda: torch_clip(torch, w, x), "new": lambda: ops.clip_search(w, x, N_BIT, N_GRID, N_STEPS)}, reps,
                {"torch": 1, "new": 3})
    row.update({"clip_" + k: v for k, v in c.items()})
    row["clip_fraction_of_2.5PFLOPs"] = round(2 * (N_STEPS + 1) * N * K * S / (c["new_ms"] * 1e-3) / PEAK_FLOPS, 4)

    # quantise + pack to cdna4
    def old_route():
        fake, s, z = torch_fake(torch, w)
        fl = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device=dev)
        fl.weight.data = fake
        return WQLinear.from_linear(fl, N_BIT, 128, False, s, z).to_cdna4()

    a, b = WQLinear.quantize_linear(lin, N_BIT, 128), old_route()
    row["quantize_same_bits"] = bool(torch.equal(a.qweight, b.qweight) and torch.equal(a.scales.view(torch.int16), b.scales.view(torch.int16))
                                     and torch.equal(a.scaled_zeros.view(torch.int16), b.scaled_zeros.view(torch.int16)))
    del a, b
    c = compare(torch, {"torch": old_route, "new": lambda: WQLinear.quantize_linear(lin, N_BIT, 128),
                        "launch_only": lambda: ops.quantize_pack(w, n_bit=N_BIT, layout="cdna4")}, reps, {"torch": 1, "new": 3})
    row.update({"quantize_" + k: v for k, v in c.items()})

    # one evaluation of the scale search's w_quantize_func(w * s) / s
    out = torch.empty_like(w)
    old_fake = lambda: torch_fake(torch, w * cs)[0] / cs
    row["fake_quant_same_bits"] = bool(torch.equal(quantize.fake_quant_scaled(w, cs).view(torch.int16), old_fake().view(torch.int16)))
    c = compare(torch, {"torch": old_fake, "new": lambda: quantize.fake_quant_scaled(w, cs, out=out)}, reps, {"torch": 3, "new": 3})
    row.update({"fake_quant_" + k: v for k, v in c.items()})

    # the two short launches again as device time: GRAPH_CALLS captured calls, device events around one replay (no launch or Python overhead)
    row.update(graph_figures(torch, {"fake_quant_torch": old_fake, "fake_quant_new": lambda: quantize.fake_quant_scaled(w, cs, out=out),
                                     "fake_quant_new_again": lambda: quantize.fake_quant_scaled(w, cs, out=out),
                                     "quantize_launch_only": lambda: ops.quantize_pack(w, n_bit=N_BIT, layout="cdna4")}, reps))
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("awq_quant_bench needs the GPU: there is no CPU timing of a GPU kernel")
    with torch.no_grad():
        for shape in a.shapes.split(","):
            N, K = (int(v) for v in shape.split("x"))
            print("ROW " + json.dumps(point(torch, N, K, a.tokens, a.reps, "cuda:0")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "awq_quant_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--shapes", a.shapes, "--tokens", str(a.tokens)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"awq_quant_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"awq_quant_bench: the measurements failed with exit status {r.returncode}; stopping")
    goals_graph = {"fake_quant_faster_than_torch_beyond_margin_at_every_shape_device_time":
                   (all(row["fake_quant_graph_faster_beyond_margin"] for row in rows) if rows else "not measured")}
    goals = {f"{kind}_faster_than_torch_beyond_margin_at_every_shape": (all(row[kind + "_faster_beyond_margin"] for row in rows) if rows else "not measured")
             for kind in ("clip", "quantize", "fake_quant")}
    goals.update(goals_graph)
    summary = dict(points=len(rows), goals=goals,
                   fake_quant_new_over_torch_device_time={f'{row["N"]}x{row["K"]}': row["fake_quant_graph_new_over_torch"] for row in rows},
                   new_over_torch={f'{row["N"]}x{row["K"]}': {k: row[k + "_new_over_torch"] for k in ("clip", "quantize", "fake_quant")} for row in rows},
                   clip_fraction_of_2_5_PFLOPs={f'{row["N"]}x{row["K"]}': row["clip_fraction_of_2.5PFLOPs"] for row in rows},
                   not_measured=["fp16", "n_bit 3", "token counts other than the one given", "the clip search and quantize_linear as device time", "hardware counters"])
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tokens=a.tokens, summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
