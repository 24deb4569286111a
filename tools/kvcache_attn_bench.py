"""Attention over the KV cache with device-side lengths (attn_kvcache, rope_kv_store_natural_pos) against the host-length calls it
replaces, on the MI355X.  Llama-3-8B's attention (H 32, Hkv 8, Dh 128), bf16, one query token.

  (a) equal    B 1, lengths 2048 / 8192 / 32768 / 131072, max_seqlen_k = the length: attn_kvcache against attn_splitkv, whose plan gives
               the same chunk there.  Prices the device-length read.
  (b) loose    lengths 8192 and 32768 under max_seqlen_k = 131072, against attn_splitkv at the length.  Prices a plan made from a loose
               bound: chunks sized for 131072 keys and a grid most of whose blocks leave at once.  No goal, a price to publish.
  (c) ragged   B 8, lengths {131072, 32768, 8192, 2048, 2048, 512, 64, inactive}: ONE attn_kvcache call against the seven per-sequence
               attn_splitkv calls it replaces (the two shortest take the one-pass kernel there, as flash_attn_func routes them).
  (c') full    B 8, every length 32768 = max_seqlen_k: the plan (sized for one sequence: chunk 1024) against a forced chunk of 4096, which
               is what counting the whole batch in the two-blocks-per-CU rule would choose.  Prices that choice where it could hurt.
  (d) store    rope_kv_store_natural_pos against rope_kv_store_natural, one token, B 1 and B 8.
  (e) fp8      (a) and (c) on the FP8 cache: attn_kvcache_kv8 against attn_splitkv_kv8.

Two timings per point, measured in one process on the same tensors, alternating.  Every figure times ONE captured graph of N calls on N
distinct tensor sets -- at least 1 GiB of attended K / V together where N <= 32 allows, so no call finds its keys in the 256 MiB
last-level cache -- replayed `reps` times; a point reports the best replay and the spread (max - min) / min of its replays.  The new
form is captured twice: the relative difference of the two identical graphs is the same-box noise the ratio is read against.

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/kvcache_attn_bench.py [--out profiles/kvcache_attn_bench.json] [--reps 5] [--only equal,loose,ragged,store,fp8]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV, DH = 32, 8, 128
EQUAL = (2048, 8192, 32768, 131072)
LOOSE = ((8192, 131072), (32768, 131072))
RAGGED = (131072, 32768, 8192, 2048, 2048, 512, 64, None)  # None: an inactive slot (-1)
GROUPS = ("equal", "loose", "ragged", "store", "fp8")
DEV = "cuda:0"
CHILD_TIMEOUT_S = 420
SCALE = DH ** -0.5


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


def time_pair(torch, new, old, n, reps):
    """new / old: functions that issue the N calls of one graph.  Returns the figures of a row."""
    graphs = {"new": graph_of(torch, new), "old": graph_of(torch, old), "new_again": graph_of(torch, new)}
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(calls_per_graph=n)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["new_over_old"] = round(best["new"] / best["old"], 4)
    row["same_box_noise"] = round(abs(best["new"] - best["new_again"]) / min(best["new"], best["new_again"]), 4)
    del graphs
    return row


def caches(torch, ops, lens, lmax, fp8):
    """(q, k, v, k_scale, v_scale, seqlens) of one set: row b holds lens[b] random keys; the rows behind them are never read."""
    B = len(lens)
    q = (1.5 * torch.randn(B, 1, H, DH, device=DEV)).to(torch.bfloat16)
    k = torch.zeros(B, lmax, HKV, DH, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros(B, lmax, HKV, DH, dtype=torch.bfloat16, device=DEV)
    for b, n in enumerate(lens):
        if n:
            k[b, :n] = torch.randn(n, HKV, DH, device=DEV)
            v[b, :n] = 1 + 0.5 * torch.randn(n, HKV, DH, device=DEV)
    sl = torch.tensor([n if n else -1 for n in lens], dtype=torch.int32, device=DEV)
    if not fp8:
        return q, k, v, None, None, sl
    (kq, ks), (vq, vs) = ops.kv8_quant(k), ops.kv8_quant(v)
    return q, kq, vq, ks, vs, sl


def attn_point(torch, E, ops, what, lens, bound, fp8, reps):
    live = [n for n in lens if n]
    kv_bytes = sum(live) * HKV * DH * 2 * (1 if fp8 else 2)
    n = max(2, min(32, -(-(1 << 30) // kv_bytes)))
    sets = [caches(torch, ops, lens, bound, fp8) for _ in range(n)]
    keep = []

    def new():
        keep.clear()
        for q, k, v, ks, vs, sl in sets:
            keep.append(E.attn_kvcache_kv8(q, k, v, ks, vs, sl, bound, 0, SCALE, True) if fp8 else E.attn_kvcache(q, k, v, sl, bound, 0, SCALE, True))

    def old():  # one host-length call per live sequence, on views of the same caches
        keep.clear()
        for q, k, v, ks, vs, sl in sets:
            for b, m in enumerate(lens):
                if not m:
                    continue
                if fp8:
                    keep.append(E.attn_splitkv_kv8(q[b:b + 1], k[b:b + 1, :m], v[b:b + 1, :m], ks[b:b + 1, :m], vs[b:b + 1, :m], SCALE, True))
                else:
                    keep.append(E.attn_splitkv(q[b:b + 1], k[b:b + 1, :m], v[b:b + 1, :m], SCALE, True))
    new()
    got = keep[0].clone()
    old()
    max_diff = max(float((got[b].float() - o[0].float()).abs().max()) for b, o in zip([b for b, m in enumerate(lens) if m], keep[:len(live)]))
    row = dict(point=what, fp8=fp8, lens=[m if m else -1 for m in lens], max_seqlen_k=bound,
               plan=list(ops.attn_kvcache_plan(len(lens), H, HKV, DH, 1, bound)),
               old_plans=[list(ops.attn_splitkv_plan(1, H, HKV, DH, 1, m, True)) for m in live], old_calls=len(live), max_abs_diff_vs_old=max_diff)
    row.update(time_pair(torch, new, old, n, reps))
    row["hbm_fraction"] = round(kv_bytes / (row["new_us"] * 1e-6) / 8e12, 4)
    del sets, keep
    torch.cuda.empty_cache()
    return row


def full_point(torch, E, ops, reps):
    from llm_awq_amd import _capi

    lens, bound, forced = (32768,) * 8, 32768, 4096
    sets = [caches(torch, ops, lens, bound, False) for _ in range(2)]
    keep = []

    def run():
        keep.clear()
        for q, k, v, ks, vs, sl in sets:
            keep.append(E.attn_kvcache(q, k, v, sl, bound, 0, SCALE, True))
    plan = list(ops.attn_kvcache_plan(8, H, HKV, DH, 1, bound))
    graphs = {"new": graph_of(torch, run)}
    _capi.tune(attn_splitkv_chunk=forced)  # the plan is read when the graph is captured
    graphs["old"] = graph_of(torch, run)
    _capi.tune(attn_splitkv_chunk=0)
    graphs["new_again"] = graph_of(torch, run)
    times = {name: [] for name in graphs}
    for _ in range(reps):
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / 2)
    best = {name: min(t) for name, t in times.items()}
    row = dict(point="full", fp8=False, lens=list(lens), max_seqlen_k=bound, plan=plan, old_chunk=forced, calls_per_graph=2)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["new_over_old"] = round(best["new"] / best["old"], 4)
    row["same_box_noise"] = round(abs(best["new"] - best["new_again"]) / min(best["new"], best["new_again"]), 4)
    del sets, keep, graphs
    torch.cuda.empty_cache()
    return row


def store_point(torch, E, B, reps):
    lmax, n = 4096, 64
    W = (H + 2 * HKV) * DH
    x = torch.randn(B, 1, W, device=DEV).to(torch.bfloat16)
    table = torch.randn(lmax, DH, device=DEV)
    kc = torch.zeros(B, lmax, HKV, DH, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    pos = 1000
    sl = torch.full((B,), pos, dtype=torch.int32, device=DEV)
    fr = table[pos:pos + 1].expand(B, DH).contiguous()  # the host form's angles of this call: [S = 1, B, rot]
    keep = []

    def new():
        keep.clear()
        for _ in range(n):
            keep.append(E.rope_kv_store_natural_pos(x, table, kc, vc, sl, H, HKV))

    def old():
        keep.clear()
        for _ in range(n):
            keep.append(E.rope_kv_store_natural(x, fr, kc, vc, pos, H, HKV))
    new()
    a = keep[0].clone()
    old()
    row = dict(point="store", B=B, same_bits=bool(torch.equal(a.view(torch.int16), keep[0].view(torch.int16))))
    row.update(time_pair(torch, new, old, n, reps))
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("kvcache_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)
    if a.group == "equal":
        for n in EQUAL:
            emit(attn_point(torch, E, ops, "equal", (n,), n, False, a.reps))
    elif a.group == "loose":
        for n, bound in LOOSE:
            emit(attn_point(torch, E, ops, "loose", (n,), bound, False, a.reps))
    elif a.group == "ragged":
        emit(attn_point(torch, E, ops, "ragged", RAGGED, max(n for n in RAGGED if n), False, a.reps))
        emit(full_point(torch, E, ops, a.reps))
    elif a.group == "store":
        for B in (1, 8):
            emit(store_point(torch, E, B, a.reps))
    elif a.group == "fp8":
        for n in EQUAL:
            emit(attn_point(torch, E, ops, "equal", (n,), n, True, a.reps))
        emit(attn_point(torch, E, ops, "ragged", RAGGED, max(n for n in RAGGED if n), True, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvcache_attn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="equal", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for group in a.only.split(","):  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"kvcache_attn_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"kvcache_attn_bench: {group} failed with exit status {r.returncode}; stopping")

    def margin(r):
        return max(r["same_box_noise"], r["new_spread"], r["old_spread"])
    judged = [r for r in rows if r["point"] in ("equal", "store")]
    ragged = [r for r in rows if r["point"] == "ragged"]
    summary = dict(points=len(rows),
                   equal_or_store_slower_beyond_noise=[(r["point"], r.get("fp8"), r.get("lens", r.get("B")), r["new_over_old"]) for r in judged
                                                       if r["new_over_old"] > 1.0 + margin(r)],
                   ragged_new_over_sum_of_old=[(r["fp8"], r["new_over_old"]) for r in ragged],
                   ragged_faster_beyond_noise=[bool(r["new_over_old"] < 1.0 - margin(r)) for r in ragged],
                   full_batch_plan_over_batch_rule=[r["new_over_old"] for r in rows if r["point"] == "full"],
                   loose_new_over_old=[(r["lens"][0], r["new_over_old"]) for r in rows if r["point"] == "loose"],
                   same_box_noise_max=max((r["same_box_noise"] for r in rows), default=None))
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, Sq=1, dtype="bfloat16"), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
