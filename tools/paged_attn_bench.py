"""The paged KV cache (attn_kvcache_paged, rope_kv_store_paged) against the dense calls it stands beside, on the MI355X.  Llama-3-8B's
attention (H 32, Hkv 8, Dh 128), bf16, one query token.

  attention   attn_kvcache_paged on a pool against attn_kvcache on the dense gather of the same data (same plan, same chunk, same bits):
              B 1 at 2048 / 8192 / 32768 / 131072 keys, and the ragged B 8 batch {131072, 32768, 8192, 2048, 2048, 512, 64, inactive};
              page sizes 64 / 256 / 1024; once with the pages in order (page i of the pool is the i-th page handed out) and once
              shuffled; the T pools and the FP8 pools.  Prices the per-tile table lookup and the loss of row-to-row contiguity.
  store       rope_kv_store_paged against rope_kv_store_natural_pos, one token, B 1 and B 8, page size 256.
  memory      no GPU: the pages the ragged batch holds against the rows of the dense rectangle.

Method of tools/kvcache_attn_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets (at least 1 GiB of
attended K / V together where N <= 32 allows) replayed `reps` times; a point reports the best replay and the spread of its replays; the two
paths alternate in one process; the paged form is captured twice, and the relative difference of the two identical graphs is the same-box
noise the ratio is read against.  A point is "slower beyond noise" when paged / dense > 1 + max(same-box noise, both spreads).

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/paged_attn_bench.py [--out profiles/paged_attn_bench.json] [--reps 5] [--only T,fp8,store] [--page-sizes 64,256,1024]
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

from kvcache_attn_bench import DEV, DH, EQUAL, H, HKV, RAGGED, SCALE, caches, time_pair  # noqa: E402

GROUPS = ("T", "fp8", "store")
CHILD_TIMEOUT_S = 540


def memory_rows():
    """Pages held by the ragged batch against the dense rectangle (rows of K, the same for V)."""
    live = [n for n in RAGGED if n]
    dense_rows = len(RAGGED) * max(live)
    out = []
    for ps in (64, 256, 1024):
        pages = sum(-(-n // ps) for n in live)
        out.append(dict(point="memory", page_size=ps, live_tokens=sum(live), pages=pages, pool_rows=pages * ps, dense_rows=dense_rows,
                        pool_over_dense=round(pages * ps / dense_rows, 4),
                        pool_gib_bf16_kv=round(pages * ps * HKV * DH * 2 * 2 / 2 ** 30, 3), dense_gib_bf16_kv=round(dense_rows * HKV * DH * 2 * 2 / 2 ** 30, 3)))
    return out


def pools_of(torch, dense, lens, ps, shuffled, seed):
    """(k_pool, v_pool, k_scale, v_scale, table) holding the live pages of one dense set, in order or shuffled."""
    q, k, v, ks, vs, sl = dense
    B, lmax = k.shape[0], k.shape[1]
    pps = lmax // ps
    mask = torch.zeros(B, pps, dtype=torch.bool, device=DEV)
    for b, n in enumerate(lens):
        if n:
            mask[b, :-(-n // ps)] = True
    P = int(mask.sum())
    ids = torch.arange(P, device=DEV)
    if shuffled:
        ids = torch.randperm(P, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    table = torch.zeros(B, pps, dtype=torch.int32, device=DEV)
    table[mask] = ids.int()

    def pool(t):
        if t is None:
            return None
        if t.dtype == torch.float8_e4m3fn:  # (indexing moves bytes: the codes travel as uint8, which the kernels take as well)
            t = t.view(torch.uint8)
        out = torch.empty(P, ps, *t.shape[2:], dtype=t.dtype, device=DEV)
        out[ids] = t.view(B, pps, ps, *t.shape[2:])[mask]
        return out
    return pool(k), pool(v), pool(ks), pool(vs), table


def attn_point(torch, E, ops, what, lens, bound, fp8, ps, shuffled, dense_sets, reps):
    live = [n for n in lens if n]
    kv_bytes = sum(live) * HKV * DH * 2 * (1 if fp8 else 2)
    n = len(dense_sets)
    paged_sets = [pools_of(torch, d, lens, ps, shuffled, i) for i, d in enumerate(dense_sets)]
    keep = []

    def new():
        keep.clear()
        for (q, _, _, _, _, sl), (kp, vp, ksp, vsp, table) in zip(dense_sets, paged_sets):
            keep.append(E.attn_kvcache_paged_kv8(q, kp, vp, ksp, vsp, table, sl, bound, 0, SCALE, True) if fp8 else
                        E.attn_kvcache_paged(q, kp, vp, table, sl, bound, 0, SCALE, True))

    def old():
        keep.clear()
        for q, k, v, ks, vs, sl in dense_sets:
            keep.append(E.attn_kvcache_kv8(q, k, v, ks, vs, sl, bound, 0, SCALE, True) if fp8 else E.attn_kvcache(q, k, v, sl, bound, 0, SCALE, True))
    new()
    got = [t.clone() for t in keep]
    old()
    same = all(bool(torch.equal(a.view(torch.int16), b.view(torch.int16))) for a, b in zip(got, keep))
    row = dict(point=what, fp8=fp8, page_size=ps, shuffled=shuffled, lens=[m if m else -1 for m in lens], max_seqlen_k=bound,
               plan=list(ops.attn_kvcache_plan(len(lens), H, HKV, DH, 1, bound)), pages=int(paged_sets[0][0].shape[0]), same_bits=same)
    row.update(time_pair(torch, new, old, n, reps))
    row["hbm_fraction"] = round(kv_bytes / (row["new_us"] * 1e-6) / 8e12, 4)
    del paged_sets, keep, got
    torch.cuda.empty_cache()
    return row


def store_point(torch, E, B, ps, reps):
    lmax, n = 4096, 64
    W = (H + 2 * HKV) * DH
    x = torch.randn(B, 1, W, device=DEV).to(torch.bfloat16)
    freqs = torch.randn(lmax, DH, device=DEV)
    kc = torch.zeros(B, lmax, HKV, DH, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    kp, vp = kc.view(-1, ps, HKV, DH).clone(), vc.view(-1, ps, HKV, DH).clone()
    table = torch.randperm(B * lmax // ps, device=DEV).int().view(B, lmax // ps)
    sl = torch.full((B,), 1000, dtype=torch.int32, device=DEV)
    keep = []

    def new():
        keep.clear()
        for _ in range(n):
            keep.append(E.rope_kv_store_paged_pos(x, freqs, kp, vp, table, sl, H, HKV))

    def old():
        keep.clear()
        for _ in range(n):
            keep.append(E.rope_kv_store_natural_pos(x, freqs, kc, vc, sl, H, HKV))
    new()
    a = keep[0].clone()
    old()
    row = dict(point="store", B=B, page_size=ps, same_bits=bool(torch.equal(a.view(torch.int16), keep[0].view(torch.int16))))
    row.update(time_pair(torch, new, old, n, reps))
    return row


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("paged_attn_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)
    sizes = [int(s) for s in a.page_sizes.split(",")]

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)
    if a.group == "store":
        for B in (1, 8):
            emit(store_point(torch, E, B, 256, a.reps))
        return
    fp8 = a.group == "fp8"
    for what, lens in [("single", (n,)) for n in EQUAL] + [("ragged", RAGGED)]:
        bound = max(n for n in lens if n)
        kv_bytes = sum(n for n in lens if n) * HKV * DH * 2 * (1 if fp8 else 2)
        n_sets = max(2, min(32, -(-(1 << 30) // kv_bytes)))
        dense_sets = [caches(torch, ops, lens, bound, fp8) for _ in range(n_sets)]  # made once per point, shared by its six paged forms
        for ps in sizes:
            for shuffled in (False, True):
                emit(attn_point(torch, E, ops, what, lens, bound, fp8, ps, shuffled, dense_sets, a.reps))
        del dense_sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_attn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--page-sizes", default="64,256,1024")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--group", default="T", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = memory_rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    for group in [g for g in a.only.split(",") if g]:  # one child per group, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--group", group, "--reps", str(a.reps), "--page-sizes", a.page_sizes]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"paged_attn_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"paged_attn_bench: {group} failed with exit status {r.returncode}; stopping")

    def margin(r):
        return max(r["same_box_noise"], r["new_spread"], r["old_spread"])
    timed = [r for r in rows if r["point"] != "memory"]
    summary = dict(points=len(timed), groups=a.only, all_same_bits=all(r["same_bits"] for r in timed),
                   slower_beyond_noise=[(r["point"], r.get("fp8"), r["page_size"], r.get("shuffled"), r.get("lens", r.get("B")), r["new_over_old"],
                                         round(margin(r), 4)) for r in timed if r["new_over_old"] > 1.0 + margin(r)],
                   paged_over_dense_max=max((r["new_over_old"] for r in timed), default=None),
                   paged_over_dense_min=min((r["new_over_old"] for r in timed), default=None),
                   same_box_noise_max=max((r["same_box_noise"] for r in timed), default=None),
                   ragged_pool_over_dense_rows={r["page_size"]: r["pool_over_dense"] for r in rows if r["point"] == "memory"})
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, Sq=1, dtype="bfloat16"), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
