"""The FP8 KV cache against the T (fp16 / bf16) cache on the MI355X, on the same values: the decode phase of the natural-layout long-context
path (a few query rows over a long history), one prompt-sized call on the one-pass kernel, and the store launch.

Shapes: Llama-3-8B's attention (H 32, Hkv 8, Dh 128) and a Dh 64 shape (H 64, Hkv 8), batch 1, Sq in {1, 8, 32}, Sk in {2048, 8192,
32768, 131072}, plus Sq = Sk = 2048 (the one-pass kernel).  Timings per point, measured in one process, alternating:

  (a) fp8   the engine's attn_splitkv_kv8 on codes + scales (csrc/awq_kv8.hpp; the one-pass attn_prefill_kv8 where the plan does not split);
  (b) t     the engine's attn_splitkv on ops.kv8_dequant of the same codes -- the tensors (a) multiplies with, so both compute the same bits.

Every figure times ONE captured graph of N calls on N distinct (q, k, v) sets -- at least 1 GiB of T-cache K / V together where N <= 32
allows, so no call finds its keys in the 256 MiB last-level cache, in either format -- replayed `reps` times; a point reports the best replay
and the spread (max - min) / min of its replays.  (a) is captured twice: the relative difference of the two identical graphs is the
same-box noise the ratio is read against.  hbm_fraction_* is (K + V bytes [+ scale bytes]) / time over 8 TB/s, a whole-call figure.

The store rows time rope_kv_store_natural_fp8 against rope_kv_store_natural on the same qkv tensors (S = 1 and S = 2048).

Each (shape, dtype) group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/kv8_attn_bench.py [--out profiles/kv8_attn_bench.json] [--reps 5] [--dtypes bfloat16,float16]
  python tools/kv8_attn_bench.py --sweep-chunk     # Llama-3-8B, bf16, Sq 1: every chunk of CHUNKS forced through the knob
                                                   # attn_splitkv_chunk, both formats; writes profiles/kv8_attn_sweep.json
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
PROMPT = (2048, 2048)
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


def timed(torch, graphs, reps, n):
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    return times


def point(torch, E, ops, H, Hkv, Dh, Sq, Sk, dtype, reps):
    t_bytes = 2 * Sk * Hkv * Dh * 2
    fp8_bytes = 2 * Sk * Hkv * (Dh + 4)
    n = max(2, min(32, -(-(1 << 30) // t_bytes)))
    sets = []
    for _ in range(n):
        q = (1.5 * torch.randn(1, Sq, H, Dh, device=DEV)).to(dtype)
        k8, ks = ops.kv8_quant(torch.randn(1, Sk, Hkv, Dh, device=DEV).to(dtype))
        v8, vs = ops.kv8_quant((1 + 0.5 * torch.randn(1, Sk, Hkv, Dh, device=DEV)).to(dtype))
        sets.append((q, k8, v8, ks, vs, ops.kv8_dequant(k8, ks, dtype), ops.kv8_dequant(v8, vs, dtype)))
    keep = []

    def run(fp8):
        def f():
            keep.clear()
            for q, k8, v8, ks, vs, kd, vd in sets:
                keep.append(E.attn_splitkv_kv8(q, k8, v8, ks, vs, Dh ** -0.5, True) if fp8 else E.attn_splitkv(q, kd, vd, Dh ** -0.5, True))
        return f

    splits, chunk = ops.attn_splitkv_plan(1, H, Hkv, Dh, Sq, Sk, True)
    q, k8, v8, ks, vs, kd, vd = sets[0]
    same_bits = bool(torch.equal(E.attn_splitkv_kv8(q, k8, v8, ks, vs, Dh ** -0.5, True).view(torch.int16),
                                 E.attn_splitkv(q, kd, vd, Dh ** -0.5, True).view(torch.int16)))
    graphs = {"fp8": graph_of(torch, run(True)), "t": graph_of(torch, run(False)), "fp8_again": graph_of(torch, run(True))}
    times = timed(torch, graphs, reps, n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(kind="attention", H=H, Hkv=Hkv, Dh=Dh, Sq=Sq, Sk=Sk, dtype=str(dtype)[6:], calls_per_graph=n, splits=splits, chunk=chunk,
               same_bits_as_t_on_dequantised=same_bits)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["fp8_over_t"] = round(best["fp8"] / best["t"], 4)
    row["byte_ratio"] = round(fp8_bytes / t_bytes, 4)
    row["same_box_noise"] = round(abs(best["fp8"] - best["fp8_again"]) / min(best["fp8"], best["fp8_again"]), 4)
    row["hbm_fraction_fp8"] = round(fp8_bytes / (best["fp8"] * 1e-6) / HBM_BYTES_PER_S, 4)
    row["hbm_fraction_t"] = round(t_bytes / (best["t"] * 1e-6) / HBM_BYTES_PER_S, 4)
    del sets, graphs, keep
    torch.cuda.empty_cache()
    return row


def store_point(torch, E, H, Hkv, Dh, S, dtype, reps):
    n = 32 if S == 1 else 8
    L = n * S
    W = (H + 2 * Hkv) * Dh
    xs = [torch.randn(1, S, W, device=DEV).to(dtype) for _ in range(n)]
    inv = 1.0 / (10000.0 ** (torch.arange(0, Dh, 2, device=DEV).float() / Dh))
    frs = []
    for i in range(n):
        f = torch.outer(torch.arange(i * S, (i + 1) * S, device=DEV).float(), inv)
        frs.append(torch.cat([f, f], -1)[None].contiguous())
    kt, vt = torch.zeros(1, L, Hkv, Dh, dtype=dtype, device=DEV), torch.zeros(1, L, Hkv, Dh, dtype=dtype, device=DEV)
    k8, v8 = torch.zeros(1, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV), torch.zeros(1, L, Hkv, Dh, dtype=torch.float8_e4m3fn, device=DEV)
    ks, vs = torch.zeros(1, L, Hkv, device=DEV), torch.zeros(1, L, Hkv, device=DEV)
    keep = []

    def run(fp8):
        def f():
            keep.clear()
            for i in range(n):
                keep.append(E.rope_kv_store_natural_fp8(xs[i], frs[i], k8, v8, ks, vs, i * S, H, Hkv) if fp8
                            else E.rope_kv_store_natural(xs[i], frs[i], kt, vt, i * S, H, Hkv))
        return f

    graphs = {"fp8": graph_of(torch, run(True)), "t": graph_of(torch, run(False)), "fp8_again": graph_of(torch, run(True))}
    times = timed(torch, graphs, reps, n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(kind="store", H=H, Hkv=Hkv, Dh=Dh, S=S, dtype=str(dtype)[6:], calls_per_graph=n)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["fp8_over_t"] = round(best["fp8"] / best["t"], 4)
    row["same_box_noise"] = round(abs(best["fp8"] - best["fp8_again"]) / min(best["fp8"], best["fp8_again"]), 4)
    del xs, graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import _capi, ops

    if not torch.cuda.is_available():
        raise SystemExit("kv8_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
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
    print("ROW " + json.dumps(point(torch, E, ops, H, Hkv, Dh, PROMPT[0], PROMPT[1], dtype, a.reps)), flush=True)
    for S in (1, 2048):
        print("ROW " + json.dumps(store_point(torch, E, H, Hkv, Dh, S, dtype, a.reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/kv8_attn_bench.json (profiles/kv8_attn_sweep.json with --sweep-chunk)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="bfloat16,float16")
    ap.add_argument("--sweep-chunk", action="store_true", help="Llama-3-8B, bf16, Sq = 1: each chunk of CHUNKS forced through the knob")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--shape", default="llama3_8b", help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="bfloat16", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    groups = [("llama3_8b", "bfloat16")] if a.sweep_chunk else [(s, d) for s in SHAPES for d in a.dtypes.split(",")]
    rows = []
    for shape, dtype in groups:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--dtype", dtype, "--reps", str(a.reps)]
        if a.sweep_chunk:
            cmd.append("--sweep-chunk")
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"kv8_attn_bench: {shape} {dtype} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"kv8_attn_bench: {shape} {dtype} failed with exit status {r.returncode}; stopping")
    if not rows:
        raise SystemExit("kv8_attn_bench: the children printed no rows; nothing is written")
    att = [r for r in rows if r["kind"] == "attention"]
    noise = lambda r: max(r["same_box_noise"], r["fp8_spread"], r["t_spread"])
    long_ = [r for r in att if r["Sk"] >= 32768]
    summary = dict(points=len(rows), dtypes=a.dtypes.split(","),
                   all_same_bits=all(r["same_bits_as_t_on_dequantised"] for r in att),
                   fp8_over_t_from_32768_keys=[min((r["fp8_over_t"] for r in long_), default=None), max((r["fp8_over_t"] for r in long_), default=None)],
                   faster_beyond_noise=[(r["H"], r["Dh"], r["Sq"], r["Sk"], r["dtype"], r.get("forced_chunk")) for r in att
                                        if r["fp8_over_t"] < 1.0 - noise(r)],
                   slower_beyond_noise=[(r["H"], r["Dh"], r["Sq"], r["Sk"], r["dtype"], r.get("forced_chunk")) for r in att
                                        if r["fp8_over_t"] > 1.0 + noise(r)],
                   same_box_noise_max=max(r["same_box_noise"] for r in rows),
                   replay_spread_max=max(r[k] for r in rows for k in r if k.endswith("_spread")))
    print(json.dumps(summary), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "kv8_attn_sweep.json" if a.sweep_chunk else "kv8_attn_bench.json")
    with open(out, "w") as f:
        json.dump(dict(shapes=SHAPES, batch=1, sweep_chunk=bool(a.sweep_chunk), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
