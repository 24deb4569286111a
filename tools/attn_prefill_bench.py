"""Prefill attention (flash_attn_func -> awq_inference_engine.attn_prefill, csrc/awq_attn_prefill_cdna4.hip) on the MI355X: time per
call, the matrix-core FLOPs of the attended pairs as a fraction of 2.5 PFLOP/s, and the ratio to two references measured in the same
process, alternating with the kernel:

  (a) eager   the composition of tinychat/modules/fused_attn.py:287-302 (repeat_interleave, [B, H, Sq, Sk] scores, fp32 softmax, second
              matmul) -- what a prompt costs without the kernel;
  (b) sdpa    torch.nn.functional.scaled_dot_product_attention(is_causal=True) with K / V expanded for GQA.

Every figure times ONE captured graph of N calls on N distinct (q, k, v) sets (N >= 32 for the kernel, so launch gaps and L2 reuse
between calls do not flatter it; the references run N = 4 because of their score tensors), replayed `reps` times; the point reports the
best replay and the spread (max - min) / min of its replays.

  python tools/attn_prefill_bench.py [--out FILE.json] [--quick] [--no-ref] [--sweep-tiles]

--sweep-tiles forces each q tile (64 / 128 / 256 rows) in turn through the tuning knob `attn_prefill_rows` (awq_tune_set, AWQ_TUNING=1)
and times the kernel alone, bf16, Sq = Sk: the measurement attn_prefill_plan was set from (profiles/attn_prefill_tile_sweep.txt).
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
from llm_awq_amd import _capi, ops  # noqa: E402

PEAK = 2.5e15
SHAPES = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128), "falcon7b_like": (64, 8, 64), "llama3_70b_tp8": (8, 1, 128)}
DEV = "cuda:0"


def attended_pairs(Sq, Sk):
    """Causal, bottom-right aligned: row i attends i + Sk - Sq + 1 keys."""
    return Sq * (Sk - Sq) + Sq * (Sq + 1) // 2


def eager(q, k, v, start_pos):
    B, Sq, H, Dh = q.shape
    G = H // k.shape[2]
    keys = torch.repeat_interleave(k, dim=2, repeats=G).transpose(1, 2)
    values = torch.repeat_interleave(v, dim=2, repeats=G).transpose(1, 2)
    xq = q.transpose(1, 2)
    scores = torch.matmul(xq, keys.transpose(2, 3)) / math.sqrt(Dh)
    mask = torch.triu(torch.full((1, 1, Sq, k.shape[1]), float("-inf"), device=q.device), diagonal=start_pos + 1).type_as(scores)
    scores = torch.softmax((scores + mask).float(), dim=-1).type_as(xq)
    return torch.matmul(scores, values).transpose(1, 2).contiguous()


def sdpa(q, k, v, start_pos):
    G = q.shape[2] // k.shape[2]
    kk = torch.repeat_interleave(k, dim=2, repeats=G).transpose(1, 2)
    vv = torch.repeat_interleave(v, dim=2, repeats=G).transpose(1, 2)
    if start_pos == 0:
        o = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk, vv, is_causal=True)
    else:  # (is_causal aligns top-left: the chunk shape takes an explicit mask)
        Sq, Sk = q.shape[1], k.shape[1]
        m = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).tril(diagonal=start_pos)
        o = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk, vv, attn_mask=m)
    return o.transpose(1, 2).contiguous()


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


def point(E, model, Sq, Sk, dtype, with_ref, reps=7):
    H, Hkv, Dh = SHAPES[model]
    n = 32
    sets = [(torch.randn(1, Sq, H, Dh, device=DEV).to(dtype), torch.randn(1, Sk, Hkv, Dh, device=DEV).to(dtype),
             torch.randn(1, Sk, Hkv, Dh, device=DEV).to(dtype)) for _ in range(n)]
    scale = Dh ** -0.5
    keep = []

    def ours():
        keep.clear()
        for q, k, v in sets:
            keep.append(E.attn_prefill(q, k, v, scale, True))

    graphs = {"kernel": (graph_of(ours), n)}
    row = dict(model=model, Sq=Sq, Sk=Sk, dtype=str(dtype)[6:], H=H, Hkv=Hkv, Dh=Dh, calls_per_graph=n)
    row["q_tile_rows"], row["blocks"] = ops.attn_prefill_plan(1, H, Hkv, Dh, Sq, Sk, True)
    if with_ref:
        m = 4
        for name, f in (("eager", eager), ("sdpa", sdpa)):
            try:
                def ref(f=f):
                    for q, k, v in sets[:m]:
                        f(q, k, v, Sk - Sq)
                graphs[name] = (graph_of(ref), m)
            except RuntimeError as e:  # (out of memory at the largest points)
                row[name + "_error"] = str(e).splitlines()[0][:120]
                torch.cuda.empty_cache()
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, (g, cnt) in graphs.items():
            times[name].append(replay_us(g) / cnt)
    us = min(times["kernel"])
    flops = 4.0 * H * Dh * attended_pairs(Sq, Sk)
    row.update(us_per_call=round(us, 2), spread=round((max(times["kernel"]) - us) / us, 4), tflops=round(flops / us / 1e6, 1),
               frac_of_2p5_pflops=round(flops / us / 1e6 / (PEAK / 1e12), 4))
    for name in ("eager", "sdpa"):
        if name in times:
            t = min(times[name])
            row[name + "_us_per_call"] = round(t, 2)
            row[name + "_spread"] = round((max(times[name]) - t) / t, 4)
            row["speedup_vs_" + name] = round(t / us, 2)
    del sets, graphs, keep
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one S = 2048 call, no references (for a profiler run)")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--sweep-tiles", action="store_true", help="kernel time with each q tile forced in turn (no references)")
    ap.add_argument("--models", default=",".join(SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_prefill_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    if a.quick:
        H, Hkv, Dh = SHAPES["llama3_8b"]
        q = torch.randn(1, 2048, H, Dh, device=DEV, dtype=torch.bfloat16)
        k = torch.randn(1, 2048, Hkv, Dh, device=DEV, dtype=torch.bfloat16)
        for _ in range(3):
            E.attn_prefill(q, k, k, Dh ** -0.5, True)
        torch.cuda.synchronize()
        return
    if a.sweep_tiles:
        for model in a.models.split(","):
            for S in (256, 512, 1024, 2048, 4096, 8192):
                res = {}
                for tile in (64, 128, 256):
                    _capi.tune(attn_prefill_rows=tile)
                    r = point(E, model, S, S, torch.bfloat16, False)
                    res[tile] = (r["us_per_call"], r["tflops"])
                _capi.tune(attn_prefill_rows=0)
                print(model, S, res, flush=True)
        return
    rows = []
    shapes = [(s, s) for s in (256, 512, 1024, 2048, 4096, 8192)] + [(512, 2560)]
    for model in a.models.split(","):
        for dtype in (torch.bfloat16, torch.float16):
            for Sq, Sk in shapes:
                r = point(E, model, Sq, Sk, dtype, not a.no_ref)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), peak_flops=PEAK, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
