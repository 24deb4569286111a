"""Sliding-window attention on a packed step (attn_paged_varq_window) against the unwindowed attn_paged_varq, on the MI355X.  Llama-3-8B's
attention (H 32, Hkv 8, Dh 128), bf16, 256-key pages, shuffled tables, window_left 4095 (a window of 4096 keys), split_seqlen_q = 1 and the
default floor (ops.ATTN_SPLIT_MIN_KEYS).  The goals were written into README.md before the run:

  (a) decode   32 one-token sequences at 32768 keys: the windowed call is faster than the unwindowed call on the same step beyond the margin,
               and no slower beyond the margin than the unwindowed call on 32 one-token sequences at 4096 keys -- the keys it attends.
  (b) chunk    the same two comparisons for one 512-token chunk that ends at 32768 keys (against one that ends at 4096).
               Published without a goal next to (a) and (b): the short unwindowed step again on the first pages of the long step's tables
               (the same keys a sequence, scattered over the eight times larger pool).
  (c) cover    32 one-token sequences at 4096 keys plus a 512-token chunk over 2048: with window_left covering everything the windowed entry
               is no slower than the existing one beyond the margin.

Method of tools/varq_split_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets; the paths of a point
alternate in one process; a figure is the best of `reps` replays with the spread of its replays; the first path is captured twice and the
relative difference of the two identical graphs is the same-box noise.  margin = max(same-box noise, the spreads of the two paths compared).
Each goal is published as met or missed with its ratio and margin; nothing here asserts a time.

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

Without a GPU (`--pages`, and at the head of every run) the tool prints the pages one 131072-token sequence holds with and without
PageTable.release_before under the scheduler's rule: host logic only.

  python tools/window_attn_bench.py [--out profiles/window_attn_bench.json] [--reps 5] [--only decode,chunk,cover] [--pages]
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

GROUPS = ("decode", "chunk", "cover")
CHILD_TIMEOUT_S = 420
LEFT = 4095
LONG, SHORT = 32768, 4096
PAGE = 256
TOKENS = 131072


def pages_held(left=LEFT, page=PAGE, tokens=TOKENS, prompt=512):
    """One sequence fed a `prompt`-token chunk, then one token a step, up to `tokens`: the most pages its slot ever holds."""
    from llm_awq_amd.paged_kv import PageTable

    out = {}
    for release in (False, True):
        pps = -(-tokens // page)
        t = PageTable(num_pages=pps, page_size=page, max_batch=1, pages_per_seq=pps, device="cpu")
        sk, most = 0, 0
        while sk < tokens:
            sk += prompt if sk == 0 else 1
            t.reserve(0, sk)
            most = max(most, len(t.pages(0)))
            if release and (sk % 64 == 0 or sk == prompt):   # the rule moves in steps of 64 keys
                t.release_before(0, max(0, sk - left) & ~63)
        out["with_release_before" if release else "without"] = dict(most_pages_held=most, pages_held_at_the_end=len(t.pages(0)))
    out["structural_bound"] = f"ceil((left + Sq_b) / page_size) + 1 = {-(-(left + prompt) // page) + 1} during the prompt, {-(-(left + 1) // page) + 1} while decoding"
    return dict(tokens=tokens, page_size=page, window_left=left, prompt_chunk=prompt, **out)


def time_paths(torch, graph_of, replay_us, paths, n, reps):
    """paths: {name: function that issues the N calls of one graph}; the first path is captured a second time for the same-box noise."""
    first = next(iter(paths))
    graphs = {name: graph_of(torch, fn) for name, fn in paths.items()}
    graphs[first + "_again"] = graph_of(torch, paths[first])
    times = {name: [] for name in graphs}
    for _ in range(reps):  # alternating
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    best = {name: min(t) for name, t in times.items()}
    row = dict(calls_per_graph=n)
    for name, t in times.items():
        row[name + "_us"] = round(best[name], 2)
        row[name + "_spread"] = round((max(t) - best[name]) / best[name], 4)
    row["same_box_noise"] = round(abs(best[first] - best[first + "_again"]) / min(best[first], best[first + "_again"]), 4)
    del graphs
    return row, best


def against(row, best, new, old):
    """new / old and the margin it is read against."""
    ratio = round(best[new] / best[old], 4)
    margin = round(max(row["same_box_noise"], row[new + "_spread"], row[old + "_spread"]), 4)
    verdict = "faster" if ratio < 1.0 - margin else ("slower" if ratio > 1.0 + margin else "within the margin")
    return dict(ratio=ratio, margin=margin, verdict=verdict)


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("window_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    from kvcache_attn_bench import DH, H, HKV, SCALE, graph_of, replay_us
    from varq_prefill_bench import PS, SETS, make_set

    assert PS == PAGE
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)
    floor = ops.ATTN_SPLIT_MIN_KEYS

    def plain(s, max_q):
        return E.attn_paged_varq(s["q"], s["kp"], s["vp"], s["table"], s["cu"], max_q, s["hist"], s["bound"], 1, floor, True, SCALE, True)

    def window(s, max_q, left=LEFT):
        return E.attn_paged_varq_window(s["q"], s["kp"], s["vp"], s["table"], s["cu"], max_q, s["hist"], s["bound"], 1, floor, left, True, SCALE, True)
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

    if a.group in ("decode", "chunk"):
        n_new, B = (1, 32) if a.group == "decode" else (512, 1)
        long_sets = [make_set(torch, [(n_new, LONG - n_new)] * B, 50 + i) for i in range(SETS)]
        short_sets = [make_set(torch, [(n_new, SHORT - n_new)] * B, 60 + i) for i in range(SETS)]
        # published without a goal: the short unwindowed step again, on the first pages of the LONG sets' tables -- the same 4096 keys a
        # sequence, scattered over a pool eight times the size, which is where the windowed call finds its keys
        wide_sets = [dict(s, hist=torch.full_like(s["hist"], SHORT - n_new), bound=SHORT) for s in long_sets]
        paths = dict(window_long=over(lambda s: window(s, n_new), long_sets), plain_long=over(lambda s: plain(s, n_new), long_sets),
                     plain_short=over(lambda s: plain(s, n_new), short_sets), plain_short_wide_pool=over(lambda s: plain(s, n_new), wide_sets))
        differs = not same_bits([window(s, n_new) for s in long_sets], [plain(s, n_new) for s in long_sets])
        row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
        row.update(point=a.group, sequences=B, new_tokens=n_new, keys_long=LONG, keys_short=SHORT, window_left=LEFT, split_min_keys=floor,
                   window_plan=list(ops.attn_varq_window_plan(B, H, HKV, DH, 1, long_sets[0]["bound"], LEFT)),
                   plain_plan=list(ops.attn_varq_split_plan(B, H, HKV, DH, 1, long_sets[0]["bound"])), window_changes_the_result=differs,
                   vs_same_step_without_a_window=against(row, best, "window_long", "plain_long"),
                   vs_unwindowed_at_the_attended_keys=against(row, best, "window_long", "plain_short"),
                   vs_unwindowed_at_the_attended_keys_in_the_wide_pool=against(row, best, "window_long", "plain_short_wide_pool"))
        emit(row)
    else:
        seqs = [(1, SHORT - 1)] * 32 + [(512, 2048)]
        sets = [make_set(torch, seqs, 70 + i) for i in range(SETS)]
        every = 2 ** 31 - 1
        paths = dict(window_cover=over(lambda s: window(s, 512, every), sets), plain=over(lambda s: plain(s, 512), sets))
        same = same_bits([window(s, 512, every) for s in sets], [plain(s, 512) for s in sets])
        row, best = time_paths(torch, graph_of, replay_us, paths, SETS, a.reps)
        row.update(point="cover", decodes=32, decode_keys=SHORT, chunk=[512, 2048], window_left=every, same_bits=same,
                   vs_existing_entry=against(row, best, "window_cover", "plain"))
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_attn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--pages", action="store_true", help="print the page count of a 131072-token sequence and stop (no GPU needed)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="decode", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    pages = pages_held()
    print(json.dumps(dict(pages=pages)), flush=True)
    if a.pages:
        return
    rows = []
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"window_attn_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"window_attn_bench: {group} failed with exit status {r.returncode}; stopping")
    by = {r["point"]: r for r in rows}
    summary = dict(points=len(rows), groups=a.only)
    for goal, point in (("a", "decode"), ("b", "chunk")):
        if point in by:
            r = by[point]
            summary[f"goal_{goal}_faster_than_the_same_step_without_a_window"] = r["vs_same_step_without_a_window"]
            summary[f"goal_{goal}_faster_met"] = r["vs_same_step_without_a_window"]["verdict"] == "faster"
            summary[f"goal_{goal}_no_slower_than_unwindowed_at_{SHORT}_keys"] = r["vs_unwindowed_at_the_attended_keys"]
            summary[f"goal_{goal}_no_slower_met"] = r["vs_unwindowed_at_the_attended_keys"]["verdict"] != "slower"
            summary[f"{point}_vs_unwindowed_at_{SHORT}_keys_in_the_wide_pool_no_goal"] = r["vs_unwindowed_at_the_attended_keys_in_the_wide_pool"]
    if "cover" in by:
        summary["goal_c_no_slower_than_the_existing_entry"] = by["cover"]["vs_existing_entry"]
        summary["goal_c_met"] = by["cover"]["vs_existing_entry"]["verdict"] != "slower"
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=32, Hkv=8, Dh=128, dtype="bfloat16", page_size=PAGE, window_left=LEFT, split_seqlen_q=1), pages=pages,
                           summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
