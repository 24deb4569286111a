"""Chunk prefill on the FT KV cache on the MI355X (llm_awq_amd/fused_attn.py: rope_kv_store -> attn_prefill_ftcache), Llama-3-8B's
attention shape (H 32, Hkv 8, Dh 128), batch 1: a question of 32 tokens over 16 / 256 / 1024 / 4096 tokens of history, and a whole
prompt of 2048 from position 0, bf16 and fp16.  Three timings per point, measured in one process, alternating:

  (a) new      the two launches: rope_kv_store, attn_prefill_ftcache over keys 0 .. start_pos + S - 1;
  (b) parent   what the same step cost before them, tinychat/modules/fused_attn.py:439-483 on this package's kernels: two
               fused_rope_with_pos_forward_func calls, the permute / contiguous of K and the two slice-assigns into the caches, the
               gather of the cached history back to [B, Sk, Hkv, Dh] for K and V, flash_attn_func;
  (c) the attention launches alone: attn_prefill_ftcache on the caches against attn_prefill on keys and values gathered beforehand.

Every figure times ONE captured graph of N steps on N distinct input sets (each with caches of its own, so no step finds the previous
one's data in L2 by construction), replayed `reps` times; a point reports the best replay and the spread (max - min) / min of its
replays.  (a) is captured twice: the relative difference of the two identical graphs is the same-box noise the ratios are read against.

  python tools/chunk_prefill_bench.py [--out profiles/chunk_prefill_bench.json] [--reps 9]
  python tools/chunk_prefill_bench.py --quick      # three cached-attention calls at history 4096 and nothing else: for a counter run
                                                   # (LDS bank conflicts, fetch size) of its own, with no tracing combined
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import llm_awq_amd  # noqa: E402

H, HKV, DH = 32, 8, 128
POINTS = [(32, 16), (32, 256), (32, 1024), (32, 4096), (2048, 0)]  # (S, history)
DEV = "cuda:0"


def freqs_of(start, n, base=500000.0):
    inv = 1.0 / (base ** (torch.arange(0, DH, 2, device=DEV).float() / DH))
    f = torch.outer(torch.arange(start, start + n, device=DEV).float(), inv)
    return torch.cat([f, f], -1)[None].contiguous()


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


def new_step(E, qkv, fr, kc, vc, pos):
    S = qkv.shape[1]
    q = E.rope_kv_store(qkv, fr, kc, vc, pos, H, HKV)
    return E.attn_prefill_ftcache(q, kc, vc, 0, pos + S, DH ** -0.5, True)


def parent_step(E, qkv, fr, kc, vc, pos):
    """short_forward with chunk_prefilling (fused_attn.py:439-483), line for line"""
    B, S, _ = qkv.shape
    x = qkv.view(B, S, H + 2 * HKV, DH)
    xq, xk, xv = x[:, :, :H], x[:, :, H:H + HKV], x[:, :, -HKV:]
    xq = E.fused_rope_with_pos_forward_func(xq, fr, True)
    xk = E.fused_rope_with_pos_forward_func(xk, fr, True)
    values_store = xv.transpose(2, 1)
    keys_store = xk.reshape(B, S, HKV, DH // 8, 8).permute(0, 2, 3, 1, 4).contiguous()
    vc[:B, :, pos:pos + S, :] = values_store
    kc[:B, :, :, pos:pos + S, :] = keys_store
    keys = kc[:, :, :, 0:pos + S, :].permute(0, 3, 1, 2, 4).reshape(B, pos + S, HKV, DH).contiguous()
    values = vc[:, :, 0:pos + S, :].transpose(2, 1).reshape(B, pos + S, HKV, DH).contiguous()
    return E.attn_prefill(xq, keys, values, DH ** -0.5, True)


def point(E, S, hist, dtype, reps, n):
    lmax = hist + S + 37  # (not a multiple of the tile)
    sets = []
    for _ in range(n):
        qkv = torch.randn(1, S, (H + 2 * HKV) * DH, device=DEV).to(dtype)
        kc = torch.randn(1, HKV, DH // 8, lmax, 8, device=DEV).to(dtype)
        vc = torch.randn(1, HKV, lmax, DH, device=DEV).to(dtype)
        sets.append((qkv, kc, vc))
    fr = freqs_of(hist, S)
    keep = []

    def run(step):
        def f():
            keep.clear()
            for qkv, kc, vc in sets:
                keep.append(step(E, qkv, fr, kc, vc, hist))
        return f

    # the attention alone: q and the gathered copies are made once, outside the graphs
    pre = []
    for qkv, kc, vc in sets:
        q = E.rope_kv_store(qkv, fr, kc, vc, hist, H, HKV)
        k = kc[:, :, :, 0:hist + S, :].permute(0, 3, 1, 2, 4).reshape(1, hist + S, HKV, DH).contiguous()
        v = vc[:, :, 0:hist + S, :].transpose(2, 1).reshape(1, hist + S, HKV, DH).contiguous()
        pre.append((q, kc, vc, k, v))
    a0, b0 = new_step(E, *sets[0][:1], fr, *sets[0][1:], hist), parent_step(E, *sets[0][:1], fr, *sets[0][1:], hist)
    same_bits = bool(torch.equal(a0.view(torch.int16), b0.view(torch.int16)))

    def attn_cached():
        keep.clear()
        for q, kc, vc, k, v in pre:
            keep.append(E.attn_prefill_ftcache(q, kc, vc, 0, hist + S, DH ** -0.5, True))

    def attn_gathered():
        keep.clear()
        for q, kc, vc, k, v in pre:
            keep.append(E.attn_prefill(q, k, v, DH ** -0.5, True))

    graphs = {"new": graph_of(run(new_step)), "parent": graph_of(run(parent_step)), "new_again": graph_of(run(new_step)),
              "attn_cached": graph_of(attn_cached), "attn_gathered": graph_of(attn_gathered)}
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(S=S, history=hist, dtype=str(dtype)[6:], steps_per_graph=n, lmax=lmax, same_bits_as_parent=same_bits)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["new_over_parent"] = round(best["new"] / best["parent"], 4)
    row["attn_cached_over_gathered"] = round(best["attn_cached"] / best["attn_gathered"], 4)
    row["same_box_noise"] = round(abs(best["new"] - best["new_again"]) / min(best["new"], best["new_again"]), 4)
    del sets, pre, graphs, keep
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="three cached-attention calls at history 4096, bf16 (for a counter run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chunk_prefill_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    if a.quick:
        S, hist = 32, 4096
        q = torch.randn(1, S, H, DH, device=DEV).to(torch.bfloat16)
        kc = torch.randn(1, HKV, DH // 8, hist + S + 37, 8, device=DEV).to(torch.bfloat16)
        vc = torch.randn(1, HKV, hist + S + 37, DH, device=DEV).to(torch.bfloat16)
        for _ in range(3):
            E.attn_prefill_ftcache(q, kc, vc, 0, hist + S, DH ** -0.5, True)
        torch.cuda.synchronize()
        return
    rows = []
    for dtype in (torch.bfloat16, torch.float16):
        for S, hist in POINTS:
            r = point(E, S, hist, dtype, a.reps, 8 if S > 256 else 32)
            rows.append(r)
            print(json.dumps(r), flush=True)
    summary = dict(new_le_parent_everywhere=all(r["new_over_parent"] <= 1.0 for r in rows),
                   max_new_over_parent=max(r["new_over_parent"] for r in rows),
                   max_attn_cached_over_gathered=max(r["attn_cached_over_gathered"] for r in rows),
                   min_attn_cached_over_gathered=min(r["attn_cached_over_gathered"] for r in rows),
                   same_box_noise_max=max(r["same_box_noise"] for r in rows),
                   replay_spread_max=max(r[k] for r in rows for k in r if k.endswith("_spread")))
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(H=H, Hkv=HKV, Dh=DH, batch=1), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
