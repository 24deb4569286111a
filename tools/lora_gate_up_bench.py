"""Multi-LoRA on the gate / up pair of Llama-3-8B's MLP (4096 -> 2 x 14336), on the MI355X: the fused expand `ops.lora_expand_gate_up` against the
composition of the existing launches it replaces, beside the fused no-LoRA launch and the torch per-adapter composition.  bf16; pool rank 16 and 64;
64 slots.

Points per rank:
  decode, B = 1, 8, 64     one-token sequences, every sequence on its own adapter (the rectangular call)
  packed                   one step of 32 decodes plus a 512-token chunk, 33 adapters (cu_seqlens_q on the device)

Per point, every path captured (N calls in one graph) and timed by device events around one replay:
  (i)   fused          forward_cdna4 on the interleaved stream (no epilogue) + lora_shrink (two slices) + lora_expand_gate_up
  (ii)  composition    the same base + a de-interleaved copy of its output + lora_shrink + lora_expand (slice_end = (F, 2F)) + silu_mul.  silu_mul takes
                       contiguous operands: for more than one row the two halves of the [T, 2F] copy are copied once more (two strided copies);
                       the path is what the entry points that existed before this kernel cost, not the cheapest composition one could write
  (iii) no_lora        mlp_gate_up_forward_cdna4: the fused base launch a step without LoRA runs
  (iv)  torch          the same base + de-interleaved copy, then per adapter: index_select of its rows, F.linear with A, two F.linear with B_gate /
                       B_up, a scale, index_add_; F.silu * up at the end.  The row indices are built BEFORE the clock starts, which flatters this
                       path: a server would have to read the step's ids on the host

Method of tools/lora_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of its
measurements; the relative difference of two measurements of the same thing (the fused path, captured twice) is the same-box noise; the margin of a
point is the largest of that noise and the spreads of the two paths compared.  The pools of a point fit the 256 MB Infinity Cache together with the
weight: every path may be flattered by hits a serving loop never sees.

Goal (set before anything was measured): (i) is faster than (ii) beyond the margin at EVERY point.  If it is not, the fused kernel has no reason to
exist.  Published without a goal: (i) / (iii), the price a LoRA step pays on the MLP's first half, and (i) / (iv).

The measurements run in a child process under a time limit.

  python tools/lora_gate_up_bench.py [--out profiles/lora_gate_up_bench.json] [--reps 5] [--ranks 16,64]
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

K, F = 4096, 14336
SLOTS = 64
CHILD_TIMEOUT_S = 900
POINTS = (("decode", 1), ("decode", 8), ("decode", 64), ("packed", 33))


def deinterleave(y2):
    t, n2 = y2.shape
    v = y2.view(t, n2 // 16, 2, 8)
    return v.transpose(1, 2).reshape(t, n2)      # [gate | up]: one copy


def point(torch, ops, eng, fused, R, kind, B, a_pool, b_pool, scaling, reps, dev):
    from kvcache_attn_bench import graph_of, replay_us
    import torch.nn.functional as Fn
    c4, s, z, szp, szh = fused
    gen = torch.Generator(device=dev).manual_seed(B + R)
    sq = [1] * B if kind == "decode" else [1] * 32 + [512]
    starts = [0]
    for q in sq:
        starts.append(starts[-1] + q)
    cu = None if kind == "decode" else torch.tensor(starts, dtype=torch.int32, device=dev)
    max_sq, total_q = max(sq), sum(sq)
    ids_host = list(range(B))
    ids = torch.tensor(ids_host, dtype=torch.int32, device=dev)
    x = torch.randn(total_q, K, device=dev, generator=gen).to(torch.bfloat16)
    ws = torch.empty(ops.lora_workspace_bytes(total_q, K, R, 2) // 4, dtype=torch.float32, device=dev)
    rows = [torch.arange(starts[b], starts[b + 1], device=dev) for b in range(B)]
    scale_host = [float(v) for v in scaling.tolist()]
    n = 10 if total_q >= 64 else 20
    keep = []

    def base():
        return eng.forward_cdna4(x, c4, s, z, szp, None, szh)

    def fused_path():
        return ops.lora_apply_gate_up(x, base(), a_pool, b_pool, scaling, ids, cu, max_sq, ws)

    def composition():
        st = deinterleave(base())
        ops.lora_apply(x, st, a_pool, b_pool, scaling, ids, (F, 2 * F), cu, max_sq, ws)
        return ops.silu_mul(st[:, :F].contiguous(), st[:, F:].contiguous())

    def no_lora():
        return eng.mlp_gate_up_forward_cdna4(x, c4, szp, szh)

    def torch_path():
        st = deinterleave(base())
        for b, a in enumerate(ids_host):
            h = Fn.linear(x.index_select(0, rows[b]), a_pool[a])
            d = torch.cat([Fn.linear(h[:, :R], b_pool[a, :F]), Fn.linear(h[:, R:], b_pool[a, F:])], 1) * scale_host[a]
            st.index_add_(0, rows[b], d)
        return Fn.silu(st[:, :F]) * st[:, F:]

    def many(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    # faster and different is not faster: the fused path must equal the composition in every bit, and stay near the torch path
    hf, hc, ht = fused_path(), composition(), torch_path()
    torch.cuda.synchronize()
    equal = bool(torch.equal(hf.view(torch.int16), hc.view(torch.int16)))
    diff_torch = float((hf.float() - ht.float()).abs().max())
    graphs = {"fused": graph_of(torch, many(fused_path)), "composition": graph_of(torch, many(composition)), "no_lora": graph_of(torch, many(no_lora)),
              "torch": graph_of(torch, many(torch_path)), "fused_again": graph_of(torch, many(fused_path))}
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(K=K, F=F, rank=R, kind=kind, B=B, total_q=total_q, dtype="bfloat16", calls_per_graph=n, plan=ops.lora_plan(K, R, 2),
               fused_equals_composition_bit_for_bit=equal, max_abs_difference_to_the_torch_path=diff_torch)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise"] = round(abs(best["fused"] - best["fused_again"]) / min(best["fused"], best["fused_again"]), 4)
    row["margin"] = max(row["same_box_noise"], row["fused_spread"], row["composition_spread"])
    row["fused_over_composition"] = round(best["fused"] / best["composition"], 4)
    row["fused_over_no_lora"] = round(best["fused"] / best["no_lora"], 4)
    row["fused_over_torch"] = round(best["fused"] / best["torch"], 4)
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    from llm_awq_amd import load_engine, ops, synth
    from llm_awq_amd.fused_mlp import QuantLlamaMLP
    from llm_awq_amd.qmodule import WQLinear

    if not torch.cuda.is_available():
        raise SystemExit("lora_gate_up_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev = "cuda:0"
    T = torch.bfloat16

    def wq(k, n, seed):
        c = synth.random_wq(k, n, dtype=T, device=dev, seed=seed, keep_q=False)
        m = WQLinear(4, 128, k, n, False, dev, dtype=T)
        m.load_state_dict(dict(qweight=c["qweight"], scales=c["scales"], scaled_zeros=c["scaled_zeros"]))
        return m

    with torch.no_grad():
        mlp = QuantLlamaMLP(wq(K, F, 1), wq(F, K, 2), wq(K, F, 3))
        mlp._build(torch.device(dev))
        eng = load_engine()
        for R in [int(r) for r in a.ranks.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(K + R)
            a_pool = torch.empty(SLOTS, 2 * R, K, dtype=T, device=dev).normal_(0.0, K ** -0.5, generator=gen)
            b_pool = torch.empty(SLOTS, 2 * F, R, dtype=T, device=dev).normal_(0.0, 0.02, generator=gen)
            scaling = torch.full((SLOTS,), 2.0, dtype=torch.float32, device=dev)
            for kind, B in POINTS:
                print("ROW " + json.dumps(point(torch, ops, eng, mlp._fused, R, kind, B, a_pool, b_pool, scaling, a.reps, dev)), flush=True)
            del a_pool, b_pool
            torch.cuda.empty_cache()


def verdicts(rows, want):
    miss = [f'r{r["rank"]}/{r["kind"]}{r["B"]}' for r in rows if not r["fused_over_composition"] < 1.0 - r["margin"]]
    differ = [f'r{r["rank"]}/{r["kind"]}{r["B"]}' for r in rows if not r["fused_equals_composition_bit_for_bit"]]
    return {"fused_faster_than_composition_beyond_the_margin_at_every_point": (not miss) if len(rows) == want else "not measured", "misses": miss,
            "points_where_the_two_paths_differ_in_a_bit": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_gate_up_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--ranks", a.ranks]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"lora_gate_up_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"lora_gate_up_bench: the measurements failed with exit status {r.returncode}; stopping")
    key = lambda r: f'r{r["rank"]}/{r["kind"]}{r["B"]}'
    summary = dict(points=len(rows), goal=verdicts(rows, len(POINTS) * len(a.ranks.split(","))),
                   fused_over_composition={key(r): r["fused_over_composition"] for r in rows},
                   fused_over_no_lora={key(r): r["fused_over_no_lora"] for r in rows},
                   fused_over_torch={key(r): r["fused_over_torch"] for r in rows},
                   fused_us={key(r): r["fused_us"] for r in rows},
                   not_measured=["fp16", "ranks other than 16 and 64", "eager (host-clock) figures", "hardware counters", "a whole model step",
                                 "a cold Infinity Cache"])
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(K=K, F=F), slots=SLOTS, summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
