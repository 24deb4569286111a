"""Split-KV attention against the one-pass prefill kernel on the MI355X: a few query rows over a long natural-layout history, the decode
phase of tinychat's long-context path (flash_attn_func(q, cache_k[:, :pos], cache_v[:, :pos], causal=True)).

Shapes: Llama-3-8B's attention (H 32, Hkv 8, Dh 128) and a Dh 64 shape (H 64, Hkv 8), batch 1, Sq in {1, 8, 32}, Sk in {2048, 8192,
32768, 131072}, bf16 and fp16.  Two timings per point, measured in one process on the same tensors, alternating:

  (a) split     the engine's attn_splitkv (csrc/awq_attn_splitkv_cdna4.hip): where its plan does not split this IS the one-pass launch;
  (b) one_pass  the engine's attn_prefill (csrc/awq_attn_prefill_cdna4.hip), which served these calls before.

Every figure times ONE captured graph of N calls on N distinct (q, k, v) sets -- at least 1 GiB of K / V together where N <= 32 allows,
so no call finds its keys in the 256 MiB last-level cache -- replayed `reps` times; a point reports the best replay and the spread
(max - min) / min of its replays.  (a) is captured twice: the relative difference of the two identical graphs is the same-box noise
the ratio is read against.  hbm_fraction is the split path's (K + V bytes) / time over 8 TB/s: a whole-call figure (both launches),
not a kernel's share of peak.

Each (shape, dtype) group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/splitkv_attn_bench.py [--out profiles/splitkv_attn_bench.json] [--reps 7]
  python tools/splitkv_attn_bench.py --sweep-chunk     # Llama-3-8B, bf16, Sq 1: every chunk of CHUNKS forced through the knob
                                                       # attn_splitkv_chunk; writes profiles/splitkv_attn_sweep.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"llama3_8b": (32, 8, 128), "dh64": (64, 8, 64)}
SQS = (1, 8, 32)
SKS = (2048, 8192, 32768, 131072)
CHUNKS = (256, 512, 1024, 2048, 4096, 8192)
DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12
CHILD_TIMEOUT_S = 420


def graph_of(torch, fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(torch, g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def point(torch, E, ops, H, Hkv, Dh, Sq, Sk, dtype, reps):
    kv_bytes = 2 * Sk * Hkv * Dh * 2
    n = max(2, min(32, -(-(1 << 30) // kv_bytes)))
    sets = []
    for _ in range(n):
        q = (1.5 * torch.randn(1, Sq, H, Dh, device=DEV)).to(dtype)
        k = torch.randn(1, Sk, Hkv, Dh, device=DEV).to(dtype)
        v = (1 + 0.5 * torch.randn(1, Sk, Hkv, Dh, device=DEV)).to(dtype)
        sets.append((q, k, v))
    keep = []

    def run(fn):
        def f():
            keep.clear()
            for q, k, v in sets:
                keep.append(fn(q, k, v, Dh ** -0.5, True))
        return f

    splits, chunk = ops.attn_splitkv_plan(1, H, Hkv, Dh, Sq, Sk, True)
    a0, b0 = E.attn_splitkv(*sets[0], Dh ** -0.5, True), E.attn_prefill(*sets[0], Dh ** -0.5, True)
    max_diff = float((a0.float() - b0.float()).abs().max())
    graphs = {"split": graph_of(torch, run(E.attn_splitkv)), "one_pass": graph_of(torch, run(E.attn_prefill)),
              "split_again": graph_of(torch, run(E.attn_splitkv))}
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(H=H, Hkv=Hkv, Dh=Dh, Sq=Sq, Sk=Sk, dtype=str(dtype)[6:], calls_per_graph=n, splits=splits, chunk=chunk,
               max_abs_diff_vs_one_pass=max_diff)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["split_over_one_pass"] = round(best["split"] / best["one_pass"], 4)
    row["same_box_noise"] = round(abs(best["split"] - best["split_again"]) / min(best["split"], best["split_again"]), 4)
    row["hbm_fraction"] = round(kv_bytes / (best["split"] * 1e-6) / HBM_BYTES_PER_S, 4)
    del sets, graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import _capi, ops

    if not torch.cuda.is_available():
        raise SystemExit("splitkv_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    H, Hkv, Dh = SHAPES[a.shape]
    dtype = getattr(torch, a.dtype)
    if a.sweep_chunk:
        for Sk in SKS:
            for c in (0,) + CHUNKS:  # 0 = the plan
                if c and c >= Sk:
                    continue
                _capi.tune(attn_splitkv_chunk=c)
                r = point(torch, E, ops, H, Hkv, Dh, 1, Sk, dtype, a.reps)
                r["forced_chunk"] = c
                print("ROW " + json.dumps(r), flush=True)
        _capi.tune(attn_splitkv_chunk=0)
        return
    for Sq in SQS:
        for Sk in SKS:
            print("ROW " + json.dumps(point(torch, E, ops, H, Hkv, Dh, Sq, Sk, dtype, a.reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/splitkv_attn_bench.json (profiles/splitkv_attn_sweep.json with --sweep-chunk)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep-chunk", action="store_true", help="Llama-3-8B, bf16, Sq = 1: each chunk of CHUNKS forced through the knob")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--shape", default="llama3_8b", help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="bfloat16", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    groups = [("llama3_8b", "bfloat16")] if a.sweep_chunk else [(s, d) for s in SHAPES for d in ("bfloat16", "float16")]
    rows = []
    for shape, dtype in groups:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--dtype", dtype, "--reps", str(a.reps)]
        if a.sweep_chunk:
            cmd.append("--sweep-chunk")
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"splitkv_attn_bench: {shape} {dtype} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"splitkv_attn_bench: {shape} {dtype} failed with exit status {r.returncode}; stopping")
    taken = [r for r in rows if r["splits"] > 1]
    summary = dict(points=len(rows), points_split=len(taken),
                   max_split_over_one_pass_where_split=max((r["split_over_one_pass"] for r in taken), default=None),
                   min_split_over_one_pass_where_split=min((r["split_over_one_pass"] for r in taken), default=None),
                   slower_beyond_noise=[(r["H"], r["Dh"], r["Sq"], r["Sk"], r["dtype"], r.get("forced_chunk")) for r in taken
                                        if r["split_over_one_pass"] > 1.0 + max(r["same_box_noise"], r["split_spread"], r["one_pass_spread"])],
                   same_box_noise_max=max(r["same_box_noise"] for r in rows),
                   replay_spread_max=max(r[k] for r in rows for k in r if k.endswith("_spread")))
    print(json.dumps(summary), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "splitkv_attn_sweep.json" if a.sweep_chunk else "splitkv_attn_bench.json")
    if out:
        with open(out, "w") as f:
            json.dump(dict(shapes=SHAPES, batch=1, sweep_chunk=bool(a.sweep_chunk), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
