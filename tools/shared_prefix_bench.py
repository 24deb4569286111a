"""Shared-prefix decode (attn_kvcache_paged_shared) against attn_kvcache_paged on the same pools and tables, on the MI355X.  Llama-3-8B's
attention (H 32, Hkv 8, Dh 128), bf16, 256-key pages, one query token: 32 sequences that share 2048 / 8192 / 32768 keys -- the same page
ids in every table row -- and hold 256 keys of their own each.

  grouped    the 32 sequences as one group of 32 (32 x G 4 = all 128 rows of the tile): the prefix is fetched once
  ungrouped  the same call with empty group arrays (no group, seq_prefix 0): what the shared entry costs a batch that shares nothing

Goals, set before anything was measured: (a) grouped is faster than attn_kvcache_paged beyond the margin at every shared length; (b)
ungrouped is no slower than attn_kvcache_paged beyond the margin.  The plan is not tuned to the outcome.

Method of tools/paged_attn_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets (at least 1 GiB of pool
rows together where N <= 32 allows) replayed `reps` times; a point reports the best replay and the spread of its replays; the two paths
alternate in one process; the new form is captured twice, and the relative difference of the two identical graphs is the same-box noise.
margin = max(same-box noise, both spreads).

Each shared length runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/shared_prefix_bench.py [--out profiles/shared_prefix_bench.json] [--reps 5] [--shared 2048,8192,32768]
  python tools/shared_prefix_bench.py --pages      (no GPU) the pages 32 samples of a 32768-token prompt hold, with and without fork
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

from kvcache_attn_bench import DEV, DH, H, HKV, SCALE, time_pair  # noqa: E402

SEQS, OWN, PS = 32, 256, 256
CHILD_TIMEOUT_S = 420


def pages_rows(prompt=32768, own=OWN, seqs=SEQS, ps=PS):
    """Pages held by `seqs` samples of one prompt after `own` tokens each, through PageTable itself."""
    from llm_awq_amd.paged_kv import PageTable

    out = {}
    for fork in (False, True):
        t = PageTable(num_pages=seqs * (prompt + own) // ps, page_size=ps, max_batch=seqs, pages_per_seq=(prompt + own) // ps, device="cpu")
        t.reserve(0, prompt)
        for s in range(1, seqs):
            if fork:
                t.fork(0, s, prompt)
            else:
                t.reserve(s, prompt)
        for s in range(seqs):
            t.reserve(s, prompt + own)
        out["fork" if fork else "no_fork"] = t.num_pages - t.free_pages
    row_bytes = HKV * DH * 2 * 2  # K and V, bf16
    return dict(point="pages", prompt=prompt, own=own, seqs=seqs, page_size=ps, pages_no_fork=out["no_fork"], pages_fork=out["fork"],
                gib_no_fork=round(out["no_fork"] * ps * row_bytes / 2 ** 30, 3), gib_fork=round(out["fork"] * ps * row_bytes / 2 ** 30, 3))


def make_set(torch, P):
    """(q, k_pool, v_pool, table, lens): P // PS shared pages named by every row, then OWN // PS pages per sequence, shuffled ids."""
    shared, own = P // PS, OWN // PS
    pages = shared + SEQS * own
    ids = torch.randperm(pages, device=DEV).int()
    table = torch.empty(SEQS, shared + own, dtype=torch.int32, device=DEV)
    table[:, :shared] = ids[:shared]
    table[:, shared:] = ids[shared:].view(SEQS, own)
    q = (1.5 * torch.randn(SEQS, 1, H, DH, device=DEV)).to(torch.bfloat16)
    kp = torch.randn(pages, PS, HKV, DH, device=DEV).to(torch.bfloat16)
    vp = (1 + 0.5 * torch.randn(pages, PS, HKV, DH, device=DEV)).to(torch.bfloat16)
    lens = torch.full((SEQS,), P + OWN, dtype=torch.int32, device=DEV)
    return q, kp, vp, table, lens


def point(torch, E, ops, P, grouped, sets, reps):
    bound = P + OWN
    gm = torch.arange(SEQS, dtype=torch.int32, device=DEV).view(1, SEQS) if grouped else torch.full((1, SEQS), -1, dtype=torch.int32, device=DEV)
    gp = torch.full((1,), P if grouped else 0, dtype=torch.int32, device=DEV)
    sp = torch.full((SEQS,), P if grouped else 0, dtype=torch.int32, device=DEV)
    keep = []

    def new():
        keep.clear()
        for q, kp, vp, table, lens in sets:
            keep.append(E.attn_kvcache_paged_shared(q, kp, vp, table, lens, bound, gm, gp, sp, P, 0, SCALE, True))

    def old():
        keep.clear()
        for q, kp, vp, table, lens in sets:
            keep.append(E.attn_kvcache_paged(q, kp, vp, table, lens, bound, 0, SCALE, True))
    new()
    got = [t.clone() for t in keep]
    old()
    same = all(bool(torch.equal(a.view(torch.int16), b.view(torch.int16))) for a, b in zip(got, keep))
    diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(got, keep))
    row = dict(point="grouped" if grouped else "ungrouped", shared=P, own=OWN, seqs=SEQS, page_size=PS, max_seqlen_k=bound,
               plan_shared=list(ops.attn_kvcache_shared_plan(SEQS, H, HKV, DH, 1, P, bound)), plan_paged=list(ops.attn_kvcache_plan(SEQS, H, HKV, DH, 1, bound)),
               same_bits=same, max_abs_diff=diff)
    row.update(time_pair(torch, new, old, len(sets), reps))
    row["margin"] = round(max(row["same_box_noise"], row["new_spread"], row["old_spread"]), 4)
    row["old_over_new"] = round(row["old_us"] / row["new_us"], 3)
    read = (P + SEQS * OWN if grouped else SEQS * bound) * HKV * DH * 2 * 2  # bytes of K / V the new call has to fetch
    row["new_hbm_fraction"] = round(read / (row["new_us"] * 1e-6) / 8e12, 4)
    row["old_hbm_fraction"] = round(SEQS * bound * HKV * DH * 2 * 2 / (row["old_us"] * 1e-6) / 8e12, 4)
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("shared_prefix_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)
    P = int(a.group)
    unique = (P + SEQS * OWN) * HKV * DH * 2 * 2
    n = max(2, min(32, -(-(1 << 30) // unique)))
    sets = [make_set(torch, P) for _ in range(n)]
    for grouped in (True, False):
        print("ROW " + json.dumps(point(torch, E, ops, P, grouped, sets, a.reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shared", default="2048,8192,32768")
    ap.add_argument("--pages", action="store_true", help="no GPU: print the pages held with and without fork and leave")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="2048", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = [pages_rows()]
    print(json.dumps(rows[0]), flush=True)
    if a.pages:
        return
    for P in [p for p in a.shared.split(",") if p]:  # one child per shared length, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", P, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"shared_prefix_bench: shared length {P} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"shared_prefix_bench: shared length {P} failed with exit status {r.returncode}; stopping")
    timed = [r for r in rows if r["point"] != "pages"]
    grouped, ungrouped = [r for r in timed if r["point"] == "grouped"], [r for r in timed if r["point"] == "ungrouped"]
    summary = dict(points=len(timed), all_same_bits=all(r["same_bits"] for r in timed),
                   paged_over_shared={r["shared"]: r["old_over_new"] for r in grouped},
                   ungrouped_over_paged={r["shared"]: r["new_over_old"] for r in ungrouped},
                   margins={f"{r['point']}-{r['shared']}": r["margin"] for r in timed},
                   goal_a_faster_beyond_margin_at_every_length=bool(grouped) and all(r["new_over_old"] < 1.0 - r["margin"] for r in grouped),
                   goal_b_ungrouped_no_slower_beyond_margin=bool(ungrouped) and all(r["new_over_old"] <= 1.0 + r["margin"] for r in ungrouped))
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, Sq=1, dtype="bfloat16", page_size=PS, seqs=SEQS, own=OWN), summary=summary, rows=rows), f,
                      indent=1)


if __name__ == "__main__":
    main()
