"""Soft-capped attention on a packed step (attn_varq_softcap) against the uncapped attn_varq_window on the SAME tensors, on the MI355X, and
the two capped LM-head epilogues against the uncapped entries.  Gemma-2-27B's attention (H 32, Hkv 16, Dh 128), bf16, dense caches, cap 50,
scale 144 ** -0.5, split_seqlen_q = 1 and the default floor (ops.ATTN_SPLIT_MIN_KEYS).  Stated before the run:

  (a) decode   GOAL: a decode step, which is memory-bound, is no slower than the uncapped call beyond the margin.  8 one-token sequences:
               window_left 4095 over 32768 keys, and a window that hides nothing over 8192 and over 32768 keys.
  (b) chunk    no goal: one 2048-token prompt chunk that ends at 8192 keys, windowed (window_left 4095) and global.  The ratio is published as
               it is; the placement of the two transcendentals inside the score loop was not tuned.
  (c) global   no goal: a global layer on the WINDOWED instantiation (attn_varq_window, a window that hides nothing) against attn_varq on the
               same step -- what not building an unwindowed softcap form costs.  The decode over 32768 keys and the chunk of (b).
  (d) head     no goal: lm_head_softcap / lm_head at M = 1 and lm_head_logprobs(softcap=30) / lm_head_logprobs at T = 2047 on Llama-3's
               matrix (V 128256, K 4096), bf16.

Method of tools/window_attn_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets; the paths of a point
alternate in one process; a figure is the best of `reps` replays with the spread of its replays; the first path is captured twice and the
relative difference of the two identical graphs is the same-box noise.  margin = max(same-box noise, the spreads of the two paths compared).
Nothing here asserts a time.  Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/softcap_attn_bench.py [--out profiles/softcap_attn_bench.json] [--reps 5] [--only decode,chunk,global,head] [--readme]
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

GROUPS = ("decode", "chunk", "global", "head")
CHILD_TIMEOUT_S = 420
H, HKV, DH = 32, 16, 128
CAP, SCALE, FINAL_CAP = 50.0, 144 ** -0.5, 30.0
LEFT = 4095
SETS = 2
DEV = "cuda:0"


def make_set(torch, seqs, seed):
    """One packed step over dense caches: q [T, H, Dh], caches [B, L, Hkv, Dh] holding hist + new keys, cu_seqlens_q, the lengths before the step."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B, L = len(seqs), max(s + h for s, h in seqs)
    kc = torch.randn(B, L, HKV, DH, device=DEV, dtype=torch.bfloat16, generator=g)
    vc = 1 + 0.5 * torch.randn(B, L, HKV, DH, device=DEV, dtype=torch.bfloat16, generator=g)
    q = (1.5 * torch.randn(sum(s for s, _ in seqs), H, DH, device=DEV, generator=g)).to(torch.bfloat16)
    cu = torch.tensor([0] + [s for s, _ in seqs], dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)
    hist = torch.tensor([h for _, h in seqs], dtype=torch.int32, device=DEV)
    return dict(q=q, kc=kc, vc=vc, cu=cu, hist=hist, bound=L)


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("softcap_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    from kvcache_attn_bench import graph_of, replay_us
    from window_attn_bench import against, time_paths

    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)
    floor = ops.ATTN_SPLIT_MIN_KEYS
    every = 2 ** 31 - 1

    def plain(s, max_q):
        return E.attn_varq(s["q"], s["kc"], s["vc"], s["cu"], max_q, s["hist"], s["bound"], 1, floor, True, SCALE, True)

    def window(s, max_q, left):
        return E.attn_varq_window(s["q"], s["kc"], s["vc"], s["cu"], max_q, s["hist"], s["bound"], 1, floor, left, True, SCALE, True)

    def softcap(s, max_q, left):
        return E.attn_varq_softcap(s["q"], s["kc"], s["vc"], s["cu"], max_q, s["hist"], s["bound"], 1, floor, left, CAP, True, SCALE, True)
    keep = []

    def over(fn, sets):
        def go():
            keep.clear()
            for s in sets:
                keep.append(fn(s))
        return go

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)

    def same_bits(x, y):
        return all(bool(torch.equal(p.view(torch.int16), q.view(torch.int16))) for p, q in zip(x, y))

    def capped_vs_window(point, seqs, max_q, left, seed):
        sets = [make_set(torch, seqs, seed + i) for i in range(SETS)]
        paths = dict(softcap=over(lambda s: softcap(s, max_q, left), sets), window=over(lambda s: window(s, max_q, left), sets))
        differs = not same_bits([softcap(s, max_q, left) for s in sets], [window(s, max_q, left) for s in sets])
        row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
        row.update(point=point, sequences=len(seqs), new_tokens=seqs[0][0], keys=seqs[0][0] + seqs[0][1], window_left=min(left, sets[0]["bound"] - 1),
                   softcap=CAP, cap_changes_the_result=differs, softcap_vs_window=against(row, best, "softcap", "window"))
        emit(row)
        del sets

    if a.group == "decode":
        capped_vs_window("decode_window_32768", [(1, 32767)] * 8, 1, LEFT, 10)
        capped_vs_window("decode_global_8192", [(1, 8191)] * 8, 1, every, 20)
        capped_vs_window("decode_global_32768", [(1, 32767)] * 8, 1, every, 30)
    elif a.group == "chunk":
        capped_vs_window("chunk_window", [(2048, 6144)], 2048, LEFT, 40)
        capped_vs_window("chunk_global", [(2048, 6144)], 2048, every, 50)
    elif a.group == "global":
        for point, seqs, max_q, seed in (("global_decode_32768", [(1, 32767)] * 8, 1, 60), ("global_chunk", [(2048, 6144)], 2048, 70)):
            sets = [make_set(torch, seqs, seed + i) for i in range(SETS)]
            paths = dict(window_cover=over(lambda s: window(s, max_q, every), sets), plain=over(lambda s: plain(s, max_q), sets))
            same = same_bits([window(s, max_q, every) for s in sets], [plain(s, max_q) for s in sets])
            row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
            row.update(point=point, sequences=len(seqs), new_tokens=seqs[0][0], keys=seqs[0][0] + seqs[0][1], same_bits=same,
                       windowed_form_vs_attn_varq=against(row, best, "window_cover", "plain"))
            emit(row)
            del sets
    else:
        V, K = 128256, 4096
        g = torch.Generator(device=DEV).manual_seed(80)
        w = (0.02 * torch.randn(V, K, device=DEV, generator=g)).to(torch.bfloat16)
        gamma = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(torch.bfloat16)
        xs = [torch.randn(1, K, device=DEV, generator=g).to(torch.bfloat16) for _ in range(SETS)]
        outs = [torch.empty(1, V, dtype=torch.float32, device=DEV) for _ in range(SETS)]
        paths = dict(softcap=lambda: [ops.lm_head_softcap(x, w, FINAL_CAP, gamma, 1e-6, out=o) for x, o in zip(xs, outs)],
                     plain=lambda: [ops.lm_head(x, w, gamma, 1e-6, out=o) for x, o in zip(xs, outs)])
        row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
        row.update(point="lm_head_m1", V=V, K=K, softcap=FINAL_CAP, softcap_vs_plain=against(row, best, "softcap", "plain"))
        emit(row)
        T = 2047
        hs = [torch.randn(T, K, device=DEV, generator=g).to(torch.bfloat16) for _ in range(SETS)]
        tg = torch.randint(0, V, (T,), device=DEV, generator=g).to(torch.int32)
        ws = torch.empty(ops.lm_head_logprobs_workspace_bytes(T, V, K, True), dtype=torch.uint8, device=DEV)
        res = [{n: torch.zeros(T, dtype=torch.float32, device=DEV) for n in ("logprob", "lse")} for _ in range(SETS)]
        paths = dict(softcap=lambda: [ops.lm_head_logprobs(h, w, tg, gamma, 1e-6, round_logits=True, ws=ws, out=o, softcap=FINAL_CAP) for h, o in zip(hs, res)],
                     plain=lambda: [ops.lm_head_logprobs(h, w, tg, gamma, 1e-6, round_logits=True, ws=ws, out=o) for h, o in zip(hs, res)])
        row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
        row.update(point="lm_head_logprobs_t2047", V=V, K=K, T=T, softcap=FINAL_CAP, softcap_vs_plain=against(row, best, "softcap", "plain"))
        emit(row)


def readme(doc):
    """The README section of a result file."""
    by = {r["point"]: r for r in doc["rows"]}
    a_pts = [p for p in ("decode_window_32768", "decode_global_8192", "decode_global_32768") if p in by]
    met = all(by[p]["softcap_vs_window"]["verdict"] != "slower" for p in a_pts)
    fmt = lambda v: f"{v['ratio']:.3f} (margin {v['margin']:.3f}: {v['verdict']})"
    worst = max(by[p]["softcap_vs_window"]["ratio"] for p in a_pts) if a_pts else float("nan")
    lines = [f"## Soft-capped attention and logits (`attn_varq_softcap`, `lm_head_softcap`): goal (a) {'met' if met else 'MISSED'} -- a capped decode step "
             f"costs up to {worst:.2f} × the uncapped one", "",
             "`tools/softcap_attn_bench.py`, Gemma-2-27B's attention (H 32 / Hkv 16 / Dh 128, bf16, cap 50, scale 144^-0.5); time of `attn_varq_softcap` over "
             "`attn_varq_window` on the same tensors, best of 5 graph replays, the margin the largest of the same-box noise and the two spreads "
             "(`profiles/softcap_attn_bench.json`).", "",
             "| point | softcap us | uncapped us | ratio |", "|---|---|---|---|"]
    for p in a_pts + [p for p in ("chunk_window", "chunk_global") if p in by]:
        r = by[p]
        lines.append(f"| {p} ({r['sequences']} x {r['new_tokens']} new over {r['keys']} keys, left {r['window_left']}) | {r['softcap_us']} | {r['window_us']} | "
                     f"{fmt(r['softcap_vs_window'])} |")
    for p in ("global_decode_32768", "global_chunk"):
        if p in by:
            r = by[p]
            lines.append(f"| {p}: windowed form, no cap, against `attn_varq` | {r['window_cover_us']} | {r['plain_us']} | {fmt(r['windowed_form_vs_attn_varq'])} |")
    for p in ("lm_head_m1", "lm_head_logprobs_t2047"):
        if p in by:
            r = by[p]
            lines.append(f"| {p} (V {r['V']}, K {r['K']}, cap 30) | {r['softcap_us']} | {r['plain_us']} | {fmt(r['softcap_vs_plain'])} |")
    lines += ["", "(a) is the goal, stated before the run: the three decode points no slower than the uncapped call beyond the margin.  The chunk, "
              "global and head rows were published without a goal; the placement of the exp2 and rcp inside the score loop was not tuned."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softcap_attn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--readme", action="store_true", help="print the README section of the result file --out names and stop (no GPU needed)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="decode", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.readme:
        print(readme(json.load(open(a.out))))
        return
    rows = []
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"softcap_attn_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"softcap_attn_bench: {group} failed with exit status {r.returncode}; stopping")
    by = {r["point"]: r for r in rows}
    summary = dict(points=len(rows), groups=a.only)
    a_pts = [p for p in ("decode_window_32768", "decode_global_8192", "decode_global_32768") if p in by]
    if a_pts:
        summary["goal_a_decode_no_slower_than_uncapped"] = {p: by[p]["softcap_vs_window"] for p in a_pts}
        summary["goal_a_met"] = all(by[p]["softcap_vs_window"]["verdict"] != "slower" for p in a_pts)
    for p in ("chunk_window", "chunk_global"):
        if p in by:
            summary[p + "_no_goal"] = by[p]["softcap_vs_window"]
    for p in ("global_decode_32768", "global_chunk"):
        if p in by:
            summary[p + "_windowed_form_vs_attn_varq_no_goal"] = by[p]["windowed_form_vs_attn_varq"]
    for p in ("lm_head_m1", "lm_head_logprobs_t2047"):
        if p in by:
            summary[p + "_no_goal"] = by[p]["softcap_vs_plain"]
    print(json.dumps(summary), flush=True)
    if a.out:
        doc = dict(shape=dict(H=H, Hkv=HKV, Dh=DH, dtype="bfloat16", softcap=CAP, softmax_scale=SCALE, window_left=LEFT, split_seqlen_q=1),
                   summary=summary, rows=rows)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
