"""The per-head q/k RMSNorm fused into the paged packed store (rope_kv_store_paged_varq[_fp8]_qknorm) on the MI355X, against the two things
it stands beside.  Qwen3-8B's attention (H 32, Hkv 8, Dh 128), bf16, 256-key pages, T and FP8 pools, three step sizes: one token, 32
sequences of one token, one 2048-token chunk.

  fused      one launch: norm, rotation, (quantisation,) store.
  composed   what the module would run without it: two slice copies (q heads, k heads out of the fused qkv rows), two `ops.rmsnorm`,
             the write-back of both into qkv, and the plain store.
  plain      the plain store on the same tokens, no norm at all: fused / plain is what the norm costs.

Goal (a), set before anything was measured: fused is faster than composed beyond the margin at every point.  (b) fused / plain is
published without a goal.

Method of tools/paged_attn_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets replayed `reps` times; a
point reports the best replay and the spread of its replays; the paths alternate in one process; the fused form is captured twice, and
the relative difference of the two identical graphs is the same-box noise.  The margin of a ratio is the largest of that noise and the
two spreads.  Each group (T, fp8) runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/qknorm_store_bench.py [--out profiles/qknorm_store_bench.json] [--reps 5] [--only T,fp8]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kvcache_attn_bench import DEV, graph_of, replay_us  # noqa: E402

H, HKV, DH, PAGE, EPS = 32, 8, 128, 256, 1e-6
GROUPS = ("T", "fp8")
# (name, sequences, tokens per sequence, tensor sets per graph)
POINTS = (("1 token", 1, 1, 64), ("32 x 1 token", 32, 1, 32), ("one 2048-token chunk", 1, 2048, 8))
CHILD_TIMEOUT_S = 300


def time_paths(torch, paths, n, reps):
    """paths: name -> function that issues the N calls of one graph; the first path is captured twice (the same-box noise)."""
    first = next(iter(paths))
    graphs = {name: graph_of(torch, fn) for name, fn in paths.items()}
    graphs[first + "_again"] = graph_of(torch, paths[first])
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    row = dict(calls_per_graph=n)
    best = {name: min(t) for name, t in times.items()}
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise"] = round(abs(best[first] - best[first + "_again"]) / min(best[first], best[first + "_again"]), 4)
    del graphs
    return row


def tensor_set(torch, B, S, fp8, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    T, W = B * S, (H + 2 * HKV) * DH
    pps = -(-(1000 + S) // PAGE) if S == 1 else -(-S // PAGE)
    pages = B * pps
    x = torch.randn(T, W, generator=g, device=DEV).to(torch.bfloat16)
    shape = (pages, PAGE, HKV, DH)
    pools = [torch.zeros(shape, dtype=torch.uint8 if fp8 else torch.bfloat16, device=DEV) for _ in range(2)]
    if fp8:
        pools += [torch.zeros(shape[:3], dtype=torch.float32, device=DEV) for _ in range(2)]
    table = torch.randperm(pages, generator=g, device=DEV).int().view(B, pps)
    lens = torch.full((B,), 1000 if S == 1 else 0, dtype=torch.int32, device=DEV)  # decodes over 1000 keys; the chunk opens its sequence
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=DEV)
    return x, pools, table, lens, cu


def point(torch, E, ops, name, B, S, n, fp8, reps):
    sfx = "_fp8" if fp8 else ""
    plain_store, fused_store = getattr(E, "rope_kv_store_paged_varq" + sfx), getattr(E, "rope_kv_store_paged_varq" + sfx + "_qknorm")
    freqs = torch.randn(4096, DH, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    gq, gk = ((1.0 + 0.1 * torch.randn(DH, device=DEV)).to(torch.bfloat16) for _ in range(2))
    gq32, gk32 = gq.float(), gk.float()
    sets = [tensor_set(torch, B, S, fp8, 100 + i) for i in range(n)]
    keep = []

    def compose_(x):  # in place, as a module would treat its own qkv: 2 slice copies, 2 norms, 2 writes back
        heads = x.view(x.shape[0], H + 2 * HKV, DH)
        q, k = heads[:, :H].contiguous(), heads[:, H:H + HKV].contiguous()
        heads[:, :H] = ops.rmsnorm(q.view(-1, DH), gq, EPS).view(-1, H, DH)
        heads[:, H:H + HKV] = ops.rmsnorm(k.view(-1, DH), gk, EPS).view(-1, HKV, DH)
        return x

    def fused():
        keep.clear()
        for x, pools, table, lens, cu in sets:
            keep.append(fused_store(x, freqs, *pools, table, cu, S, lens, H, HKV, gq32, gk32, EPS))

    def composed():
        keep.clear()
        for x, pools, table, lens, cu in sets:
            keep.append(plain_store(compose_(x), freqs, *pools, table, cu, S, lens, H, HKV))

    def plain():
        keep.clear()
        for x, pools, table, lens, cu in sets:
            keep.append(plain_store(x, freqs, *pools, table, cu, S, lens, H, HKV))
    # the bits first, on the first set: fused on x against the plain store on a composed copy
    x, pools, table, lens, cu = sets[0]
    got_q = fused_store(x, freqs, *pools, table, cu, S, lens, H, HKV, gq32, gk32, EPS)
    got = [p.clone() for p in pools]
    want_q = plain_store(compose_(x.clone()), freqs, *pools, table, cu, S, lens, H, HKV)
    torch.cuda.synchronize()
    same = bool(torch.equal(got_q.view(torch.int16), want_q.view(torch.int16))) and \
        all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(got, pools))
    row = dict(point=name, fp8=fp8, sequences=B, tokens_per_sequence=S, page_size=PAGE, same_bits=same)
    row.update(time_paths(torch, dict(fused=fused, composed=composed, plain=plain), n, reps))
    row["margin"] = round(max(row["same_box_noise"], row["fused_spread"], row["composed_spread"]), 4)
    row["fused_over_composed"] = round(row["fused_us"] / row["composed_us"], 4)
    row["fused_over_plain"] = round(row["fused_us"] / row["plain_us"], 4)
    row["margin_plain"] = round(max(row["same_box_noise"], row["fused_spread"], row["plain_spread"]), 4)
    row["goal_a_met"] = bool(row["fused_over_composed"] < 1.0 - row["margin"])
    del sets, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("qknorm_store_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)
    for name, B, S, n in POINTS:
        print("ROW " + json.dumps(point(torch, E, ops, name, B, S, n, a.group == "fp8", a.reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qknorm_store_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="T", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"qknorm_store_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"qknorm_store_bench: {group} failed with exit status {r.returncode}; stopping")
    summary = dict(points=len(rows), groups=a.only, all_same_bits=all(r["same_bits"] for r in rows),
                   goal_a="fused faster than composed beyond the margin at every point", goal_a_met=bool(rows) and all(r["goal_a_met"] for r in rows),
                   goal_a_missed_at=[(r["point"], r["fp8"], r["fused_over_composed"], r["margin"]) for r in rows if not r["goal_a_met"]],
                   fused_over_composed_max=max((r["fused_over_composed"] for r in rows), default=None),
                   fused_over_plain={("fp8 " if r["fp8"] else "T ") + r["point"]: r["fused_over_plain"] for r in rows},
                   not_measured=["fp16", "Dh 64", "dense caches", "hardware counters", "a whole model step"])
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, dtype="bfloat16", page_size=PAGE, eps=EPS), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
