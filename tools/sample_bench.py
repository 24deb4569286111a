"""Choosing the next token, on the MI355X: the one launch `ops.sample_logits` against the torch composition of the reference's loop
(tinychat/stream_generators/stream_gen.py:19-32,120-134) on the same logits.  V = 128256 (Llama-3), bf16; B = 1, 8, 64; three modes:

  greedy       temperature 0: an argmax
  topk_topp    temperature 0.7, top-p 0.95, top-k 50
  penalty      the same with repetition penalty 1.3 over a history of 512 tokens

Per point:
  torch            temperature / repetition penalty / sort-based top-p / top-k / softmax / multinomial as torch calls, eager, no host read
  torch_read       the same followed by the loop's int() of the token (B = 1) / a .tolist() (B > 1)
  device           ops.sample_logits, eager                                    (+ a second measurement of the same thing)
  device_graph     the same captured into one hipGraph of N calls, replayed    (the torch composition is measured eager only)

Method of tools/paged_attn_bench.py: the paths alternate in one process, a figure is the best of `reps` measurements and carries the spread of
its measurements, and the relative difference of two measurements of the same thing is the same-box noise a ratio is read against.  An eager
figure is a host clock around N calls that end in a device synchronise; a graph figure is device events around one replay of N captured calls.

Goal (set before anything was measured): at B = 1 the launch is faster than the torch composition WITHOUT the host read, beyond same-box noise,
in all three modes.  One block works on a row, so the passes of a row run one after the other: 1 pass for greedy, 6 for top-k + top-p (max, four
radix-select passes, the kept sums) and the same with a penalty.

The measurements run in a child process under a time limit.

  python tools/sample_bench.py [--out profiles/sample_bench.json] [--reps 5] [--batches 1,8,64]
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

V, HIST = 128256, 512
MODES = {"greedy": dict(t=0.0, p=1.0, k=0, r=1.0), "topk_topp": dict(t=0.7, p=0.95, k=50, r=1.0), "penalty": dict(t=0.7, p=0.95, k=50, r=1.3)}
PASSES = {"greedy": 1, "topk_topp": 6, "penalty": 6}
CHILD_TIMEOUT_S = 540


def torch_compose(torch, logits, hist, m):
    """the reference's processors and draw, written out as the torch calls they make (no host read)"""
    x = logits.float()
    if m["t"] >= 1e-5 and m["t"] != 1.0:
        x = x / m["t"]
    if m["r"] > 1.0:
        s = torch.gather(x, 1, hist)
        x = x.scatter(1, hist, torch.where(s < 0, s * m["r"], s / m["r"]))
    if m["t"] < 1e-5 or m["p"] < 1e-8:
        return torch.argmax(x, dim=-1)
    if 1e-8 <= m["p"] < 1.0:
        sl, si = torch.sort(x, descending=False)
        cp = sl.softmax(dim=-1).cumsum(dim=-1)
        rm = cp <= (1 - m["p"])
        rm[..., -1:] = False
        x = x.masked_fill(rm.scatter(1, si, rm), float("-inf"))
    if m["k"] > 0:
        x = x.masked_fill(x < torch.topk(x, m["k"])[0][..., -1, None], float("-inf"))
    return torch.multinomial(torch.softmax(x, dim=-1), num_samples=1)


def eager_us(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def point(torch, ops, B, mode, reps, dev):
    from kvcache_attn_bench import graph_of, replay_us
    m = MODES[mode]
    gen = torch.Generator(device=dev).manual_seed(B)
    logits = (torch.randn(B, V, device=dev, generator=gen) * 3.5).to(torch.bfloat16)
    hist = torch.randint(0, V, (B, HIST), device=dev, generator=gen)
    u = torch.rand(B, device=dev, generator=gen)
    f = dict(dtype=torch.float32, device=dev)
    kw = dict(temperature=torch.full((B,), m["t"], **f), top_p=torch.full((B,), m["p"], **f), top_k=torch.full((B,), m["k"], dtype=torch.int32, device=dev))
    if m["r"] > 1.0:
        kw.update(repetition_penalty=torch.full((B,), m["r"], **f), history=hist.int().contiguous(), hist_len=torch.full((B,), HIST, dtype=torch.int32, device=dev))
    n = 100 if B <= 8 else 30
    keep = []

    def device():
        return ops.sample_logits(logits, u, **kw)

    def n_device():
        keep.clear()
        for _ in range(n):
            keep.append(device())

    def torch_read():
        t = torch_compose(torch, logits, hist, m)
        return int(t) if B == 1 else t.tolist()
    eager = {"torch": lambda: torch_compose(torch, logits, hist, m), "torch_read": torch_read, "device": device, "device_again": device}
    graphs = {"device_graph": graph_of(torch, n_device), "device_graph_again": graph_of(torch, n_device)}
    for fn in eager.values():  # warm-up
        eager_us(torch, fn, 3)
    times = {name: [] for name in list(eager) + list(graphs)}
    for _ in range(reps):  # alternating
        for name, fn in eager.items():
            times[name].append(eager_us(torch, fn, n))
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(batch=B, mode=mode, vocab=V, passes_per_row=PASSES[mode], calls_per_measurement=n)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise_eager"] = round(abs(best["device"] - best["device_again"]) / min(best["device"], best["device_again"]), 4)
    row["same_box_noise_graph"] = round(abs(best["device_graph"] - best["device_graph_again"]) / min(best["device_graph"], best["device_graph_again"]), 4)
    row["device_over_torch"] = round(best["device"] / best["torch"], 4)
    row["device_over_torch_read"] = round(best["device"] / best["torch_read"], 4)
    row["device_graph_over_torch"] = round(best["device_graph"] / best["torch"], 4)
    row["margin_eager"] = max(row["same_box_noise_eager"], row["torch_spread"], row["device_spread"])
    del graphs, keep
    torch.cuda.empty_cache()
    return row


def child(a):
    import torch

    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs the GPU: there is no CPU timing of a GPU kernel")
    torch.manual_seed(0)
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            for mode in MODES:
                print("ROW " + json.dumps(point(torch, ops, B, mode, a.reps, "cuda:0")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--batches", a.batches]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"sample_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            rows.append(json.loads(line[4:]))
            print(line[4:], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"sample_bench: the measurements failed with exit status {r.returncode}; stopping")
    one = [r for r in rows if r["batch"] == 1]
    summary = dict(points=len(rows),
                   goal_b1_faster_than_torch_without_read_beyond_noise=(all(r["device_over_torch"] < 1.0 - r["margin_eager"] for r in one) if one else "not measured"),
                   device_over_torch={f'{r["batch"]}/{r["mode"]}': r["device_over_torch"] for r in rows},
                   device_graph_over_torch={f'{r["batch"]}/{r["mode"]}': r["device_graph_over_torch"] for r in rows},
                   margin_eager={f'{r["batch"]}/{r["mode"]}': r["margin_eager"] for r in rows})
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(V=V, dtype="bfloat16", history=HIST, modes=MODES), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
