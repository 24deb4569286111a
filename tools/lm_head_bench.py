"""The LM head of a decode step, on the MI355X: the one launch `ops.lm_head` (final RMSNorm fused, fp32 logits) against the torch composition
`ops.rmsnorm` + `torch.nn.functional.linear` + `.float()` on the same tensors.  Shapes: Llama-3-8B (V 128256, K 4096) and Llama-2-7B (V 32000,
K 4096), bf16, M = 1, 8, 64.

Per point:
  torch / torch_graph            rmsnorm -> F.linear -> .float(), eager / captured into one hipGraph of N calls and replayed
  lm_head / lm_head_graph        ops.lm_head(x, W, gamma, eps), eager / captured                     (+ a second measurement of the same thing each)

Method of tools/sample_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of its
measurements, and the relative difference of two measurements of the same thing is the same-box noise a ratio is read against.  An eager figure is
a host clock around N calls that end in a device synchronise; a graph figure is device events around one replay of N captured calls.  Every call
of a measurement reads the same weight matrix: Llama-3's 1.05 GB is four times the 256 MB Infinity Cache, Llama-2's 262 MB about fills it, so the
Llama-2 figures of BOTH paths may be flattered by cache hits a serving loop (which reads 3.7 GB of other weights between two LM heads) never sees.

Goals (set before anything was measured), judged per point on the graph figures and on the eager ones:
  (a) at M = 1 and M = 8 the new launch is no slower than the torch composition beyond the point's margin, the margin being the largest of the
      same-box noise and the two spreads;
  (b) the launch's time at M = 64 is within that margin of its time at M = 1 (the weights are read once).
Reported without a threshold: the fraction of 8 TB/s, 2 V K bytes / time / 8e12.

The measurements run in a child process under a time limit.

  python tools/lm_head_bench.py [--out profiles/lm_head_bench.json] [--reps 5] [--batches 1,8,64] [--models llama3_8b,llama2_7b]

--logprobs measures scoring instead (profiles/lm_head_logprobs_bench.json): `ops.lm_head_logprobs(x, W, targets, round_logits=True)` against the
reference's composition on the same tensors, F.linear -> .contiguous().float() -> F.cross_entropy(reduction="none"), at T = 1, 8, 64, 512 and 2047
(the perplexity window), and `ops.token_logprobs` against torch.log_softmax(...).gather on fp32 logits at B = 1, 8, 64.  Same method, graph figures
only (device events around a replay of captured calls); margin = the largest of the same-box noise and the two spreads.  Goal, set before anything
was measured: (a) at T = 2047 the fused pair is no slower than the composition beyond the point's margin, on both matrices.  Reported without a
threshold: the other row counts, 2 T V K flops / time as a fraction of 2.5 PFLOP/s, and the peak extra memory of each path (the
torch.cuda.max_memory_allocated delta of one torch call; the workspace size of ours).

  python tools/lm_head_bench.py --logprobs [--rows 1,8,64,512,2047] [--reps 5] [--models llama3_8b,llama2_7b]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODELS = {"llama3_8b": dict(V=128256, K=4096), "llama2_7b": dict(V=32000, K=4096)}
EPS = 1e-5
HBM_BYTES_PER_S = 8e12
CHILD_TIMEOUT_S = 540


def eager_us(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def point(torch, ops, model, w, gamma, M, reps, dev):
    from kvcache_attn_bench import graph_of, replay_us
    import torch.nn.functional as F
    V, K = MODELS[model]["V"], MODELS[model]["K"]
    gen = torch.Generator(device=dev).manual_seed(M)
    x = torch.randn(M, K, device=dev, generator=gen).to(torch.bfloat16)
    n = 20
    keep = []

    def new():
        return ops.lm_head(x, w, gamma, EPS)

    def old():
        return F.linear(ops.rmsnorm(x, gamma, EPS), w).float()

    def many(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    # faster and different is not faster: the two paths' logits on the tensors that are timed
    a, b = new(), old()
    diff = float((a - b).abs().max())
    eager = {"torch": old, "lm_head": new, "lm_head_again": new}
    graphs = {"torch_graph": graph_of(torch, many(old)), "lm_head_graph": graph_of(torch, many(new)), "lm_head_graph_again": graph_of(torch, many(new))}
    for fn in eager.values():  # warm-up
        eager_us(torch, fn, 3)
    times = {name: [] for name in list(eager) + list(graphs)}
    for _ in range(reps):  # alternating
        for name, fn in eager.items():
            times[name].append(eager_us(torch, fn, n))
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(model=model, V=V, K=K, M=M, dtype="bfloat16", calls_per_measurement=n, weight_bytes=2 * V * K, plan=ops.lm_head_plan(M, V, K),
               max_abs_difference_of_the_two_paths=diff)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise_eager"] = round(abs(best["lm_head"] - best["lm_head_again"]) / min(best["lm_head"], best["lm_head_again"]), 4)
    row["same_box_noise_graph"] = round(abs(best["lm_head_graph"] - best["lm_head_graph_again"]) / min(best["lm_head_graph"], best["lm_head_graph_again"]), 4)
    row["margin_eager"] = max(row["same_box_noise_eager"], row["torch_spread"], row["lm_head_spread"])
    row["margin_graph"] = max(row["same_box_noise_graph"], row["torch_graph_spread"], row["lm_head_graph_spread"])
    row["lm_head_over_torch_eager"] = round(best["lm_head"] / best["torch"], 4)
    row["lm_head_over_torch_graph"] = round(best["lm_head_graph"] / best["torch_graph"], 4)
    for name in ("lm_head", "lm_head_graph", "torch", "torch_graph"):
        row[name + "_fraction_of_8TBps"] = round(2 * V * K / (best[name] * 1e-6) / HBM_BYTES_PER_S, 4)
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("lm_head_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev = "cuda:0"
    with torch.no_grad():
        for model in a.models.split(","):
            V, K = MODELS[model]["V"], MODELS[model]["K"]
            gen = torch.Generator(device=dev).manual_seed(V)
            w = torch.empty(V, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02, generator=gen)
            gamma = (1.0 + 0.1 * torch.randn(K, device=dev, generator=gen)).to(torch.bfloat16)
            for M in [int(b) for b in a.batches.split(",")]:
                print("ROW " + json.dumps(point(torch, ops, model, w, gamma, M, a.reps, dev)), flush=True)
            del w
            torch.cuda.empty_cache()


# ---- --logprobs: the fused LM head + log-sum-exp (ops.lm_head_logprobs) against the reference's composition on the same tensors ----

PEAK_FLOPS = 2.5e15


def _timed(torch, fns, n, reps):
    """fns: name -> function issuing ONE call; each is captured n times into a graph; the graphs are replayed alternately, best of reps"""
    from kvcache_attn_bench import graph_of, replay_us
    keep = []

    def many(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    graphs = {name: graph_of(torch, many(fn)) for name, fn in fns.items()}
    times = {name: [] for name in graphs}
    for _ in range(reps):
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    spread = {name: (max(t) - best[name]) / best[name] for name, t in times.items()}
    del graphs, keep
    torch.cuda.empty_cache()
    return best, spread


def _peak_extra_bytes(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def logprobs_point(torch, ops, model, w, T, reps, dev):
    """T rows: ops.lm_head_logprobs(round_logits=True) against F.linear -> .contiguous().float() -> F.cross_entropy(reduction="none")"""
    import torch.nn.functional as F
    V, K = MODELS[model]["V"], MODELS[model]["K"]
    gen = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(T, K, device=dev, generator=gen).to(torch.bfloat16)
    tg = torch.randint(0, V, (T,), device=dev, generator=gen)
    tg32 = tg.int()
    ws = torch.empty(ops.lm_head_logprobs_workspace_bytes(T, V, K), dtype=torch.uint8, device=dev)
    out = {"logprob": torch.zeros(T, device=dev)}

    def new():
        return ops.lm_head_logprobs(x, w, tg32, round_logits=True, ws=ws, want=("logprob",), out=out)["logprob"]

    def old():
        return F.cross_entropy(F.linear(x, w).contiguous().float(), tg, reduction="none")

    diff = float((new() + old()).abs().max())        # logprob = -NLL
    n = 3 if T >= 512 else 10
    best, spread = _timed(torch, {"torch": old, "fused": new, "fused_again": new}, n, reps)
    row = dict(kind="lm_head_logprobs", model=model, V=V, K=K, T=T, dtype="bfloat16", calls_per_graph=n, plan=ops.lm_head_logprobs_plan(T, V, K),
               max_abs_difference_of_the_two_paths=diff)
    for name in best:
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round(spread[name], 4)
    row["same_box_noise"] = round(abs(best["fused"] - best["fused_again"]) / min(best["fused"], best["fused_again"]), 4)
    row["margin"] = max(row["same_box_noise"], row["torch_spread"], row["fused_spread"])
    row["fused_over_torch"] = round(best["fused"] / best["torch"], 4)
    for name in ("fused", "torch"):
        row[name + "_fraction_of_2.5PFLOPs"] = round(2.0 * T * V * K / (best[name] * 1e-6) / PEAK_FLOPS, 4)
    row["torch_peak_extra_bytes"] = _peak_extra_bytes(torch, old)
    row["fused_workspace_bytes"] = int(ws.numel())
    return row


def token_logprobs_point(torch, ops, model, B, reps, dev):
    """existing fp32 logits [B, V]: ops.token_logprobs against torch.log_softmax(...).gather"""
    V = MODELS[model]["V"]
    gen = torch.Generator(device=dev).manual_seed(B)
    logits = torch.randn(B, V, device=dev, generator=gen) * 3.0
    tg = torch.randint(0, V, (B,), device=dev, generator=gen)
    tg32 = tg.int()
    out = {"logprob": torch.zeros(B, device=dev)}

    def new():
        return ops.token_logprobs(logits, tg32, want=("logprob",), out=out)["logprob"]

    def old():
        return torch.log_softmax(logits, -1).gather(1, tg[:, None])[:, 0]

    diff = float((new() - old()).abs().max())
    best, spread = _timed(torch, {"torch": old, "rows": new, "rows_again": new}, 20, reps)
    row = dict(kind="token_logprobs", model=model, V=V, B=B, dtype="float32", calls_per_graph=20, max_abs_difference_of_the_two_paths=diff)
    for name in best:
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round(spread[name], 4)
    row["same_box_noise"] = round(abs(best["rows"] - best["rows_again"]) / min(best["rows"], best["rows_again"]), 4)
    row["margin"] = max(row["same_box_noise"], row["torch_spread"], row["rows_spread"])
    row["rows_over_torch"] = round(best["rows"] / best["torch"], 4)
    return row


def child_logprobs(a):
    import torch

    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("lm_head_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev = "cuda:0"
    with torch.no_grad():
        for model in a.models.split(","):
            V, K = MODELS[model]["V"], MODELS[model]["K"]
            gen = torch.Generator(device=dev).manual_seed(V)
            w = torch.empty(V, K, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02, generator=gen)
            for T in [int(b) for b in a.rows.split(",")]:
                print("ROW " + json.dumps(logprobs_point(torch, ops, model, w, T, a.reps, dev)), flush=True)
            del w
            torch.cuda.empty_cache()
            for B in (1, 8, 64):
                print("ROW " + json.dumps(token_logprobs_point(torch, ops, model, B, a.reps, dev)), flush=True)


def logprobs_verdicts(rows):
    """goal (a): at T = 2047 the fused pair is no slower than the composition beyond the point's margin, on both matrices"""
    out = {}
    for model in MODELS:
        r = [x for x in rows if x["kind"] == "lm_head_logprobs" and x["model"] == model and x["T"] == 2047]
        out[f"{model}/a_no_slower_than_the_composition_at_t2047"] = (r[0]["fused_over_torch"] <= 1.0 + r[0]["margin"]) if r else "not measured"
    return out


def verdicts(rows):
    """goals (a) and (b) per model and per way of measuring; "not measured" where a point is missing"""
    out = {}
    for model in sorted({r["model"] for r in rows}):
        by_m = {r["M"]: r for r in rows if r["model"] == model}
        for kind, t in (("eager", "lm_head_us"), ("graph", "lm_head_graph_us")):
            ratio, margin = "lm_head_over_torch_" + kind, "margin_" + kind
            a = [by_m[m][ratio] <= 1.0 + by_m[m][margin] for m in (1, 8) if m in by_m]
            out[f"{model}/{kind}/a_no_slower_than_torch_at_m1_m8"] = all(a) if len(a) == 2 else "not measured"
            if 1 in by_m and 64 in by_m:
                m = max(by_m[1][margin], by_m[64][margin])
                out[f"{model}/{kind}/m64_over_m1"] = round(by_m[64][t] / by_m[1][t], 4)
                out[f"{model}/{kind}/b_m64_within_margin_of_m1"] = by_m[64][t] <= by_m[1][t] * (1.0 + m)
            else:
                out[f"{model}/{kind}/b_m64_within_margin_of_m1"] = "not measured"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_head_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--models", default="llama3_8b,llama2_7b")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--logprobs", action="store_true", help="measure ops.lm_head_logprobs / ops.token_logprobs against the torch compositions "
                    "(default --out profiles/lm_head_logprobs_bench.json)")
    ap.add_argument("--rows", default="1,8,64,512,2047", help="--logprobs: the row counts T")
    a = ap.parse_args()
    if a.logprobs and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "lm_head_logprobs_bench.json")
    if a.child:
        return child_logprobs(a) if a.logprobs else child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--batches", a.batches, "--models", a.models]
    if a.logprobs:
        cmd += ["--logprobs", "--rows", a.rows]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"lm_head_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"lm_head_bench: the measurements failed with exit status {r.returncode}; stopping")
    if a.logprobs:
        fused = [r for r in rows if r["kind"] == "lm_head_logprobs"]
        summary = dict(points=len(rows), goals=logprobs_verdicts(rows),
                       fused_over_torch={f'{r["model"]}/T{r["T"]}': r["fused_over_torch"] for r in fused},
                       fused_fraction_of_peak={f'{r["model"]}/T{r["T"]}': r["fused_fraction_of_2.5PFLOPs"] for r in fused},
                       extra_bytes={f'{r["model"]}/T{r["T"]}': dict(torch=r["torch_peak_extra_bytes"], fused=r["fused_workspace_bytes"]) for r in fused},
                       rows_over_torch={f'{r["model"]}/B{r["B"]}': r["rows_over_torch"] for r in rows if r["kind"] == "token_logprobs"},
                       not_measured=["fp16", "vocabularies other than 128256 and 32000", "hardware counters", "the norm in front (gamma)", "eager calls"])
        print(json.dumps(summary), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(shapes=MODELS, summary=summary, rows=rows), f, indent=1)
        return
    summary = dict(points=len(rows), goals=verdicts(rows),
                   lm_head_over_torch_graph={f'{r["model"]}/M{r["M"]}': r["lm_head_over_torch_graph"] for r in rows},
                   lm_head_over_torch_eager={f'{r["model"]}/M{r["M"]}': r["lm_head_over_torch_eager"] for r in rows},
                   lm_head_graph_fraction_of_8TBps={f'{r["model"]}/M{r["M"]}': r["lm_head_graph_fraction_of_8TBps"] for r in rows},
                   not_measured=["fp16", "vocabularies other than 128256 and 32000", "hardware counters", "a cold Infinity Cache"])
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shapes=MODELS, eps=EPS, summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
