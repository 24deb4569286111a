"""Decode attention (awq_inference_engine.single_query_attention, csrc/awq_attn_cdna4.hip) on the MI355X: time per call,
algorithmic bytes and the fraction of 8 TB/s, next to the eager torch composition a user would otherwise write.

Every point times ONE captured graph of N calls on N distinct cache pairs (N >= 32, and enough that the K/V the calls read totals
>= 512 MiB: the set cannot stay in the 256 MiB Infinity Cache between replays), replayed with events.

  python tools/attn_decode_bench.py [--out FILE.json] [--quick] [--no-torch]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import llm_awq_amd  # noqa: E402
from llm_awq_amd import ops  # noqa: E402

PEAK = 8.0e12
SHAPES = {"llama3_8b": (32, 8, 128), "llama3_70b_tp8": (8, 1, 128)}


def alg_bytes(B, H, Hkv, Dh, L):
    """K + V of positions first_step .. tlength - 1 (read), q / k / v in, out, the k / v cache write (2 bytes per element)."""
    kv_read = 2 * B * Hkv * (L - 1) * Dh * 2
    return kv_read + (B * H * Dh * 2) * 2 + (B * Hkv * Dh * 2) * 2 * 2


def torch_composition(q, kc, vc, t, G):
    """Gather from the FT layout, matmul, softmax, matmul (fp32 softmax), the eager path without this kernel."""
    B, H, Dh = q.shape
    Hkv = vc.shape[1]
    K = kc[:B, :, :, :t + 1, :].permute(0, 1, 3, 2, 4).reshape(B, Hkv, t + 1, Dh)
    V = vc[:B, :, :t + 1, :]
    K = K.repeat_interleave(G, 1)
    V = V.repeat_interleave(G, 1)
    s = torch.matmul(q.unsqueeze(2), K.transpose(-1, -2)).float() / math.sqrt(Dh)
    p = torch.softmax(s, -1).to(q.dtype)
    return torch.matmul(p, V).squeeze(2)


def time_graph(fn, reps=5):
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
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3)
    return best


def point(E, model, B, L, dtype, with_torch):
    H, Hkv, Dh = SHAPES[model]
    dev = "cuda:0"
    kv_call = 2 * B * Hkv * L * Dh * 2
    n = max(32, math.ceil(512 * 2 ** 20 / kv_call))
    q = torch.randn(B, H, Dh, device=dev).to(dtype)
    k = torch.randn(B, Hkv, Dh, device=dev).to(dtype)
    v = torch.randn(B, Hkv, Dh, device=dev).to(dtype)
    kcs = [torch.randn(B, Hkv, Dh // 8, L, 8, device=dev).to(dtype) for _ in range(n)]
    vcs = [torch.randn(B, Hkv, L, Dh, device=dev).to(dtype) for _ in range(n)]
    t = L - 1
    outs = []

    def calls():
        outs.clear()
        for i in range(n):
            outs.append(E.single_query_attention(q, k, v, kcs[i], vcs[i], None, None, t, Dh, 500000.0, 1.0, True))

    us = time_graph(calls) / n
    nbytes = alg_bytes(B, H, Hkv, Dh, L)
    splits, chunk = ops.attn_decode_plan(B, Hkv, Dh, t, L)
    row = dict(model=model, B=B, L=L, dtype=str(dtype)[6:], H=H, Hkv=Hkv, Dh=Dh, calls_per_graph=n, splits=splits, chunk=chunk,
               us_per_call=round(us, 3), alg_bytes=nbytes, tbps=round(nbytes / us / 1e6, 3), frac_of_8tbps=round(nbytes / us / 1e6 / 8.0, 4))
    if with_torch:
        m = min(n, 8)
        try:
            def tcalls():
                for i in range(m):
                    torch_composition(q, kcs[i], vcs[i], t, H // Hkv)
            row["torch_us_per_call"] = round(time_graph(tcalls) / m, 3)
            row["speedup_vs_torch"] = round(row["torch_us_per_call"] / us, 2)
        except RuntimeError as e:  # (out of memory at the largest points)
            row["torch_us_per_call"] = None
            row["torch_error"] = str(e).splitlines()[0][:120]
    del kcs, vcs
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="two points (for a profiler run)")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    E = llm_awq_amd.install_as_awq_inference_engine()
    pts = [(m, B, L) for m in SHAPES for B in (1, 8) for L in (512, 2048, 8192, 32768)]
    if a.quick:
        pts = [("llama3_8b", 1, 8192), ("llama3_70b_tp8", 1, 32768)]
    rows = []
    for m, B, L in pts:
        r = point(E, m, B, L, torch.bfloat16, not a.no_torch)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
