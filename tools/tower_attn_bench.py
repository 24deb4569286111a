"""Encoder-tower attention (csrc/awq_attn_tower_cdna4.hip) on the MI355X at the two vision towers' shapes, against what a user had
before it, all measured in one process, alternating:

  siglip     SigLIP-so400m (fused_siglipdecoder.py:162-168): H 16, Dh 72, S 729, B 1 and 8, dense, q / k / v views of one qkv buffer
                 kernel   flash_attn_func -> attn_prefill at Dh = 72
                 sdpa     torch.nn.functional.scaled_dot_product_attention on the same views
                 pad128   zero-pad q / k / v to Dh = 128, the Dh = 128 prefill kernel with softmax_scale = 72 ** -0.5, slice, copies included
  internvit  InternViT-300M (internvit.py:45-90): H 16, Dh 64, S 1025, B 1 and 8, one packed qkv [B S, 3, H, Dh] and cu_seqlens
                 kernel   flash_attn_varlen_qkvpacked_func -> attn_varlen_qkvpacked
                 sdpa     as above, on the [B, S] view of the same (equal-length) data
                 dense64  the Dh = 64 prefill kernel on that view

Every figure times ONE captured graph of N calls on N distinct inputs, replayed `reps` times in turn with the others; a point reports
the best replay and the spread (max - min) / min.  With --sweep-tiles the kernel is also timed with each q tile (32 / 64 / 128 rows)
forced through the `tower_rows` knob (awq_tune_set, AWQ_TUNING=1): the measurement awq_attn_varlen_plan is set from.  The goal of the
kernel: no slower than sdpa, and faster than pad128; the JSON states per point whether it is met.

  python tools/tower_attn_bench.py [--out profiles/tower_attn_bench.json] [--sweep-tiles] [--reps 7]
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
from llm_awq_amd import _capi, ops  # noqa: E402

DEV = "cuda:0"
TOWERS = {"siglip": (16, 72, 729), "internvit": (16, 64, 1025)}


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


def sdpa(q, k, v):
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).contiguous()


def candidates(E, tower, B, dtype, n):
    """name -> function that runs all n calls; the inputs are n distinct buffers."""
    H, Dh, S = TOWERS[tower]
    scale = Dh ** -0.5
    keep = []
    if tower == "siglip":
        bufs = [torch.randn(B, S, 3 * H * Dh, device=DEV).to(dtype) for _ in range(n)]
        views = [tuple(b[:, :, i * H * Dh:(i + 1) * H * Dh].view(B, S, H, Dh) for i in range(3)) for b in bufs]

        def kernel():
            keep[:] = [E.attn_prefill(q, k, v, scale, False) for q, k, v in views]

        def pad128():
            keep[:] = [E.attn_prefill(F.pad(q, (0, 56)), F.pad(k, (0, 56)), F.pad(v, (0, 56)), scale, False)[..., :Dh].contiguous()
                       for q, k, v in views]

        other = {"pad128": pad128}
    else:
        bufs = [torch.randn(B * S, 3, H, Dh, device=DEV).to(dtype) for _ in range(n)]
        cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=DEV)
        views = [tuple(b.view(B, S, 3, H, Dh)[:, :, i] for i in range(3)) for b in bufs]

        def kernel():
            keep[:] = [E.attn_varlen_qkvpacked(b, cu, S, scale, False) for b in bufs]

        def dense64():
            keep[:] = [E.attn_prefill(q, k, v, scale, False) for q, k, v in views]

        other = {"dense64": dense64}

    def ref():
        keep[:] = [sdpa(q, k, v) for q, k, v in views]

    return dict(kernel=kernel, sdpa=ref, **other), (bufs, views, keep)


def point(E, tower, B, dtype, reps, sweep):
    H, Dh, S = TOWERS[tower]
    n = 32 if B == 1 else 8
    fns, hold = candidates(E, tower, B, dtype, n)
    row = dict(tower=tower, B=B, H=H, Dh=Dh, S=S, dtype=str(dtype)[6:], calls_per_graph=n)
    row["q_tile_rows"], row["blocks"] = ops.attn_varlen_plan(B, H, Dh, S)
    graphs = {}
    for name, fn in fns.items():
        try:
            graphs[name] = graph_of(fn)
        except RuntimeError as e:
            row[name + "_error"] = str(e).splitlines()[0][:160]
    if sweep:
        for rows in (32, 64, 128):
            _capi.tune(tower_rows=rows)
            graphs[f"kernel_rows{rows}"] = graph_of(fns["kernel"])  # the tile is chosen when the launch is recorded
        _capi.tune(tower_rows=0)
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(g) / n)
    for name, t in times.items():
        row[name + "_us"] = round(min(t), 2)
        row[name + "_spread"] = round((max(t) - min(t)) / min(t), 4)
    us = row["kernel_us"]
    row["tflops"] = round(4.0 * B * H * S * S * Dh / us / 1e6, 1)  # the products the algorithm needs, not the padded ones
    old = "pad128" if tower == "siglip" else "dense64"
    if "sdpa_us" in row:
        row["speedup_vs_sdpa"] = round(row["sdpa_us"] / us, 3)
    if old + "_us" in row:
        row["speedup_vs_" + old] = round(row[old + "_us"] / us, 3)
    row["goal_no_slower_than_sdpa"] = ("sdpa_us" in row and us <= row["sdpa_us"]) if "sdpa_us" in row else None
    if tower == "siglip":
        row["goal_faster_than_pad128"] = us < row["pad128_us"] if "pad128_us" in row else None
    del graphs, fns, hold
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_attn_bench.json"))
    ap.add_argument("--sweep-tiles", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tower_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    rows = []
    for tower in TOWERS:
        for B in (1, 8):
            for dtype in (torch.float16, torch.bfloat16):
                r = point(E, tower, B, dtype, a.reps, a.sweep_tiles)
                rows.append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), method="one captured graph of calls_per_graph calls per candidate, replayed "
                       f"{a.reps} times in turn; best replay, spread = (max - min) / min", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
