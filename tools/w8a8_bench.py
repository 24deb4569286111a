"""The W8A8 linear (awq_inference_engine.w8a8_gemm_fuse_bias_forward_cuda, csrc/awq_w8a8_cdna4.hip) on the MI355X for the vision towers'
shapes: time per call, 2 M N K / time as a fraction of 5 POP/s, and the ratio to torch.nn.functional.linear in fp16 with bias on the same
shape, measured in the same process, alternating with the kernel -- what a tower costs without this path.

  5 POP/s is SPEC-DERIVED AND UNMEASURED: twice the 2.5 PFLOP/s dense bf16 peak, the int8 MFMA's rate per clock relative to bf16.

Every figure times ONE captured graph of N = 32 calls on 32 distinct (x, w, out) sets (so launch gaps and cache reuse between calls do not
flatter it), after a warm-up that brings the clocks up, replayed `reps` times alternating between the two graphs; a point reports the best
replay and the spread (max - min) / min of its replays.

The layer figure is the whole encoder layer without attention and residuals:
  ours  rms_norm_general -> qkv -> invoke_quant -> out -> rms_norm_general -> fc1 -> gelu_and_quant -> fc2
  fp16  layer_norm -> qkv -> out -> layer_norm -> fc1 -> gelu(tanh) -> fc2

  python tools/w8a8_bench.py [--out FILE.json] [--quick]        (writes profiles/w8a8_bench.json by default)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import llm_awq_amd  # noqa: E402
from llm_awq_amd import ops  # noqa: E402

PEAK_OPS = 5.0e15  # spec-derived, unmeasured (see the module docstring)
DEV = "cuda:0"
# (hidden, ffn) and the row counts of one image batch: SigLIP-so400m 729 patches x {1, 8}, InternViT-300M 1025 tokens x {1, 8}
TOWERS = {"siglip_so400m": (1152, 4304, (729, 5832)), "internvit_300m": (1024, 4096, (1025, 8200))}
N_CALLS = 32


def linears(hidden, ffn):
    return [("qkv", 3 * hidden, hidden), ("out", hidden, hidden), ("fc1", ffn, hidden), ("fc2", hidden, ffn)]


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):  # warm-up to clock
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(graphs, reps):
    """graphs: {name: (graph, calls)} -> {name: (best us per call, spread)}."""
    times = {k: [] for k in graphs}
    for _ in range(reps):
        for k, (g, cnt) in graphs.items():
            times[k].append(replay_us(g) / cnt)
    return {k: (min(v), (max(v) - min(v)) / min(v)) for k, v in times.items()}


def gemm_point(E, tower, name, m, n, k, reps):
    xs = [torch.randint(-128, 128, (m, k), dtype=torch.int8, device=DEV) for _ in range(N_CALLS)]
    ws = [torch.randint(-128, 128, (n, k), dtype=torch.int8, device=DEV) for _ in range(N_CALLS)]
    outs = [torch.empty(m, n, dtype=torch.float16, device=DEV) for _ in range(N_CALLS)]
    wsc = torch.rand(n, device=DEV).mul_(1e-3).half()
    asc = torch.rand(m, device=DEV).mul_(1e-2).half()
    bias = torch.randn(n, device=DEV).half()
    xh = [torch.randn(m, k, device=DEV).half() for _ in range(N_CALLS)]
    wh = [torch.randn(n, k, device=DEV).half().mul_(0.02) for _ in range(N_CALLS)]
    keep = []

    def ours():
        for x, w, o in zip(xs, ws, outs):
            E.w8a8_gemm_fuse_bias_forward_cuda(x, w, wsc, asc, o, bias)

    def ref():
        keep.clear()
        for x, w in zip(xh, wh):
            keep.append(F.linear(x, w, bias))

    res = alternate({"w8a8": (graph_of(ours), N_CALLS), "fp16": (graph_of(ref), N_CALLS)}, reps)
    blocks, tm, tn = ops.w8a8_gemm_plan(m, n, k)
    (us, spread), (rus, rspread) = res["w8a8"], res["fp16"]
    ops_ = 2.0 * m * n * k
    row = dict(tower=tower, linear=name, M=m, N=n, K=k, tile=tm, blocks=blocks, calls_per_graph=N_CALLS, us_per_call=round(us, 2),
               spread=round(spread, 4), tops=round(ops_ / us / 1e6, 1), frac_of_5_pops_spec_unmeasured=round(ops_ / us / 1e6 / (PEAK_OPS / 1e12), 4),
               fp16_linear_us_per_call=round(rus, 2), fp16_linear_spread=round(rspread, 4), speedup_vs_fp16_linear=round(rus / us, 3))
    # the goal: no slower than the fp16 linear beyond the spreads the tool itself reports
    row["goal_met"] = bool(us <= rus * (1.0 + max(spread, rspread)))
    del xs, ws, outs, xh, wh, keep
    torch.cuda.empty_cache()
    return row


def layer_point(E, tower, m, hidden, ffn, reps, calls=8):
    eps = 1e-6
    L = linears(hidden, ffn)

    def make():
        d = dict(h=torch.randn(m, hidden, device=DEV).half(), attn=torch.randn(m, hidden, device=DEV).half(),
                 g=torch.ones(hidden, device=DEV).half(), b=torch.zeros(hidden, device=DEV).half(),
                 xq=torch.empty(m, hidden, dtype=torch.int8, device=DEV), aq=torch.empty(m, ffn, dtype=torch.int8, device=DEV),
                 scale=torch.empty(m, dtype=torch.float16, device=DEV), tmp=torch.empty(m, ffn, dtype=torch.float16, device=DEV))
        for name, n, k in L:
            d["w8_" + name] = torch.randint(-128, 128, (n, k), dtype=torch.int8, device=DEV)
            d["ws_" + name] = torch.rand(n, device=DEV).mul_(1e-3).half()
            d["wh_" + name] = torch.randn(n, k, device=DEV).half().mul_(0.02)
            d["b_" + name] = torch.randn(n, device=DEV).half().mul_(0.1)
            d["o_" + name] = torch.empty(m, n, dtype=torch.float16, device=DEV)
        return d

    sets = [make() for _ in range(calls)]
    keep = []

    def gemm(d, name, xq):
        E.w8a8_gemm_fuse_bias_forward_cuda(xq, d["w8_" + name], d["ws_" + name], d["scale"], d["o_" + name], d["b_" + name])

    def ours():
        for d in sets:
            E.rms_norm_general(d["xq"], d["h"], d["g"], d["b"], d["scale"], eps, True)
            gemm(d, "qkv", d["xq"])
            E.invoke_quant(d["xq"], d["attn"], d["scale"])
            gemm(d, "out", d["xq"])
            E.rms_norm_general(d["xq"], d["o_out"], d["g"], d["b"], d["scale"], eps, True)
            gemm(d, "fc1", d["xq"])
            E.gelu_and_quant(d["aq"], d["o_fc1"], d["scale"], d["tmp"])
            gemm(d, "fc2", d["aq"])

    def ref():
        keep.clear()
        for d in sets:
            x = F.layer_norm(d["h"], (hidden,), d["g"], d["b"], eps)
            keep.append(F.linear(x, d["wh_qkv"], d["b_qkv"]))
            o = F.linear(d["attn"], d["wh_out"], d["b_out"])
            x = F.layer_norm(o, (hidden,), d["g"], d["b"], eps)
            a = F.gelu(F.linear(x, d["wh_fc1"], d["b_fc1"]), approximate="tanh")
            keep.append(F.linear(a, d["wh_fc2"], d["b_fc2"]))

    res = alternate({"w8a8": (graph_of(ours), calls), "fp16": (graph_of(ref), calls)}, reps)
    (us, spread), (rus, rspread) = res["w8a8"], res["fp16"]
    row = dict(tower=tower, layer_without_attention=True, M=m, hidden=hidden, ffn=ffn, layers_per_graph=calls, us_per_layer=round(us, 2),
               spread=round(spread, 4), fp16_us_per_layer=round(rus, 2), fp16_spread=round(rspread, 4), speedup_vs_fp16=round(rus / us, 3))
    del sets, keep
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w8a8_bench.json"))
    ap.add_argument("--quick", action="store_true", help="three calls of one shape and nothing else (for a profiler run)")
    ap.add_argument("--shape", default="5832,4304,1152", help="M,N,K of the --quick calls")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8a8_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    if a.quick:
        m, n, k = (int(v) for v in a.shape.split(","))
        x = torch.randint(-128, 128, (m, k), dtype=torch.int8, device=DEV)
        w = torch.randint(-128, 128, (n, k), dtype=torch.int8, device=DEV)
        o = torch.empty(m, n, dtype=torch.float16, device=DEV)
        s = torch.ones(max(m, n), device=DEV).half()
        for _ in range(3):
            E.w8a8_gemm_fuse_bias_forward_cuda(x, w, s[:n], s[:m], o, s[:n])
        torch.cuda.synchronize()
        return
    rows = []
    for tower, (hidden, ffn, ms) in TOWERS.items():
        for m in ms:
            for name, n, k in linears(hidden, ffn):
                r = gemm_point(E, tower, name, m, n, k, a.reps)
                rows.append(r)
                print(json.dumps(r), flush=True)
            r = layer_point(E, tower, m, hidden, ffn, a.reps)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), peak_ops_spec_derived_unmeasured=PEAK_OPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
