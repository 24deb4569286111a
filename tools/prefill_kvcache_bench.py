"""Prompt chunks on the device-length and paged KV caches (attn_prefill_kvcache, attn_prefill_paged) against what stood there before, on the
MI355X.  Llama-3-8B's attention (H 32, Hkv 8, Dh 128), bf16.

  (a) single   one sequence, a chunk of 512 / 2048 tokens over 0 / 2048 / 32768 tokens of history: attn_prefill_kvcache and
               attn_prefill_paged (page 64 and 256, shuffled table) against attn_prefill on the same keys with the host length -- the same
               kernel body, the same q tile, the same bits.  The T caches and the FP8 caches (against attn_prefill_kv8).  Prices the
               length load and the per-tile table lookup on a compute-bound kernel.
  (b) fill     a 2048-token prompt into an empty paged pool in ONE rope_kv_store_paged + ONE attn_prefill_paged, against the only way the
               paged path had before: 64 pieces of 32 tokens through rope_kv_store_paged + attn_kvcache_paged (the split pair).
  (c) ragged   a batch of 4 with histories 0 / 512 / 8192 / inactive and a 256-token chunk each in one call, against the three
               per-sequence host-length calls.

Method of tools/paged_attn_bench.py: every figure times ONE captured graph of N calls on N distinct tensor sets replayed `reps` times; a point
reports the best replay and the spread of its replays; the two paths alternate in one process; the new form is captured twice, and the
relative difference of the two identical graphs is the same-box noise the ratio is read against.  A point is "slower beyond noise" when
new / old > 1 + max(same-box noise, both spreads).

Each group runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/prefill_kvcache_bench.py [--out profiles/prefill_kvcache_bench.json] [--reps 5] [--only T,fp8,fill,ragged]
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
from paged_attn_bench import pools_of  # noqa: E402

GROUPS = ("T", "fp8", "fill", "ragged")
CHILD_TIMEOUT_S = 540
CHUNKS, HISTORIES = (512, 2048), (0, 2048, 32768)
PAGE_SIZES = (64, 256)
SETS = 4                      # distinct tensor sets per graph
FILL_PROMPT, FILL_PIECE = 2048, 32
RAGGED_HIST, RAGGED_CHUNK = (0, 512, 8192, None), 256   # None: an inactive slot


def _round_up(n, m):
    return -(-n // m) * m


def dense_set(torch, ops, totals, Sq, fp8):
    """(q, k, v, k_scale, v_scale, total lengths) of one set: row b holds totals[b] random keys in caches whose length is a multiple of
    every page size; an inactive row holds -1."""
    B = len(totals)
    lmax = _round_up(max(n for n in totals if n), max(PAGE_SIZES))
    q = (1.5 * torch.randn(B, Sq, H, DH, device=DEV)).to(torch.bfloat16)
    k = torch.zeros(B, lmax, HKV, DH, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros_like(k)
    for b, n in enumerate(totals):
        if n:
            k[b, :n] = torch.randn(n, HKV, DH, device=DEV)
            v[b, :n] = 1 + 0.5 * torch.randn(n, HKV, DH, device=DEV)
    sl = torch.tensor([n if n else -1 for n in totals], dtype=torch.int32, device=DEV)
    if not fp8:
        return q, k, v, None, None, sl
    (kq, ks), (vq, vs) = ops.kv8_quant(k), ops.kv8_quant(v)
    return q, kq, vq, ks, vs, sl


def _new_call(E, fp8, q, k, v, ks, vs, sl, bound, table=None):
    if table is None:
        return E.attn_prefill_kvcache_kv8(q, k, v, ks, vs, sl, bound, 0, SCALE, True) if fp8 else E.attn_prefill_kvcache(q, k, v, sl, bound, 0, SCALE, True)
    return E.attn_prefill_paged_kv8(q, k, v, ks, vs, table, sl, bound, 0, SCALE, True) if fp8 else \
        E.attn_prefill_paged(q, k, v, table, sl, bound, 0, SCALE, True)


def _old_call(E, fp8, q, k, v, ks, vs, n):
    """The host-length one-pass kernel on the first n keys of a one-sequence cache."""
    if fp8:
        return E.attn_prefill_kv8(q, k[:, :n], v[:, :n], ks[:, :n], vs[:, :n], SCALE, True)
    return E.attn_prefill(q, k[:, :n], v[:, :n], SCALE, True)


def compare(torch, new, old, keep, n, reps, **row):
    new()
    got = [t.clone() for t in keep]
    old()
    row["same_bits"] = all(bool(torch.equal(a.view(torch.int16), b.view(torch.int16))) for a, b in zip(got, keep))
    row.update(time_pair(torch, new, old, n, reps))
    return row


def single_points(torch, E, ops, fp8, reps, emit):
    for chunk in CHUNKS:
        for hist in HISTORIES:
            total = hist + chunk
            sets = [dense_set(torch, ops, (total,), chunk, fp8) for _ in range(SETS)]
            flops = 4.0 * H * DH * (chunk * hist + chunk * (chunk + 1) / 2)   # the causal triangle of the chunk and the full history
            keep = []

            def old():
                keep.clear()
                for q, k, v, ks, vs, sl in sets:
                    keep.append(_old_call(E, fp8, q, k, v, ks, vs, total))
            forms = [("dense", None)] + [(f"paged{ps}", ps) for ps in PAGE_SIZES]
            for form, ps in forms:
                paged = [pools_of(torch, d, (total,), ps, True, i) for i, d in enumerate(sets)] if ps else None

                def new():
                    keep.clear()
                    for i, (q, k, v, ks, vs, sl) in enumerate(sets):
                        if paged is None:
                            keep.append(_new_call(E, fp8, q, k, v, ks, vs, sl, total))
                        else:
                            kp, vp, ksp, vsp, table = paged[i]
                            keep.append(_new_call(E, fp8, q, kp, vp, ksp, vsp, sl, total, table))
                row = compare(torch, new, old, keep, SETS, reps, point="single", goal="a", fp8=fp8, form=form, chunk=chunk, history=hist,
                              q_tile=ops.attn_prefill_plan(1, H, HKV, DH, chunk, total)[0])
                row["new_tflops"] = round(flops / (row["new_us"] * 1e-6) / 1e12, 1)
                emit(row)
                del paged
                torch.cuda.empty_cache()
            del sets
            torch.cuda.empty_cache()


def fill_point(torch, E, ops, ps, reps):
    """One store + one attention call for the whole prompt against 64 pieces of 32 tokens, both into an empty pool of their own."""
    W = (H + 2 * HKV) * DH
    pps = FILL_PROMPT // ps
    freqs = torch.randn(FILL_PROMPT, DH, device=DEV)
    sets = []
    for i in range(2):
        x = torch.randn(1, FILL_PROMPT, W, device=DEV).to(torch.bfloat16)
        pools = [torch.zeros(pps, ps, HKV, DH, dtype=torch.bfloat16, device=DEV) for _ in range(4)]  # K / V of the new path, K / V of the pieces
        table = torch.randperm(pps, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)).int().view(1, pps)
        pos = [torch.full((1,), p, dtype=torch.int32, device=DEV) for p in range(0, FILL_PROMPT, FILL_PIECE)]
        sets.append((x, pools, table, pos))
    keep = []

    def new():
        keep.clear()
        for x, (kp, vp, _, _), table, pos in sets:
            xq = E.rope_kv_store_paged_pos(x, freqs, kp, vp, table, pos[0], H, HKV)
            keep.append(E.attn_prefill_paged(xq, kp, vp, table, pos[0], FILL_PROMPT, FILL_PROMPT, SCALE, True))

    def old():
        keep.clear()
        for x, (_, _, kp, vp), table, pos in sets:
            outs = []
            for i, p in enumerate(pos):
                piece = x[:, i * FILL_PIECE:(i + 1) * FILL_PIECE]
                xq = E.rope_kv_store_paged_pos(piece, freqs, kp, vp, table, p, H, HKV)
                outs.append(E.attn_kvcache_paged(xq, kp, vp, table, p, FILL_PROMPT, FILL_PIECE, SCALE, True))
            keep.append(torch.cat(outs, 1))
    new()
    got = [t.clone() for t in keep]
    old()
    same_pools = all(bool(torch.equal(p[0].view(torch.int16), p[2].view(torch.int16)) and torch.equal(p[1].view(torch.int16), p[3].view(torch.int16)))
                     for _, p, _, _ in sets)
    diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(got, keep))
    row = dict(point="fill", goal="b", page_size=ps, prompt=FILL_PROMPT, piece=FILL_PIECE, pieces=FILL_PROMPT // FILL_PIECE, same_pools=same_pools,
               max_abs_diff_of_outputs=round(diff, 6))   # (one pass against the split pair: the same mathematics, not the same bits)
    row.update(time_pair(torch, new, old, len(sets), reps))
    return row


def ragged_points(torch, E, ops, reps, emit):
    totals = tuple(h + RAGGED_CHUNK if h is not None else None for h in RAGGED_HIST)
    bound = max(n for n in totals if n)
    sets = [dense_set(torch, ops, totals, RAGGED_CHUNK, False) for _ in range(SETS)]
    keep = []

    def old():  # the three live sequences, one host-length call each
        keep.clear()
        for q, k, v, ks, vs, sl in sets:
            keep.append(torch.cat([_old_call(E, False, q[b:b + 1], k[b:b + 1], v[b:b + 1], None, None, n) if n else torch.zeros_like(q[b:b + 1])
                                   for b, n in enumerate(totals)], 0))
    for form, ps in [("dense", None), ("paged256", 256)]:
        paged = [pools_of(torch, d, totals, ps, True, i) for i, d in enumerate(sets)] if ps else None

        def new():
            keep.clear()
            for i, (q, k, v, ks, vs, sl) in enumerate(sets):
                if paged is None:
                    keep.append(_new_call(E, False, q, k, v, None, None, sl, bound))
                else:
                    kp, vp, _, _, table = paged[i]
                    keep.append(_new_call(E, False, q, kp, vp, None, None, sl, bound, table))
        # (the plan takes B: the batch of 4 and the single calls may run different q tiles, so equal bits are reported, not required)
        emit(compare(torch, new, old, keep, SETS, reps, point="ragged", goal="c", form=form, chunk=RAGGED_CHUNK,
                     histories=[h if h is not None else -1 for h in RAGGED_HIST],
                     q_tile_batch=ops.attn_prefill_plan(len(totals), H, HKV, DH, RAGGED_CHUNK, bound)[0],
                     q_tile_single=ops.attn_prefill_plan(1, H, HKV, DH, RAGGED_CHUNK, bound)[0]))
        del paged
        torch.cuda.empty_cache()


def child(a):
    import torch

    import llm_awq_amd
    from llm_awq_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("prefill_kvcache_bench needs the GPU: there is no CPU timing of a GPU kernel")
    E = llm_awq_amd.install_as_awq_inference_engine()
    torch.manual_seed(0)

    def emit(row):
        print("ROW " + json.dumps(row), flush=True)
    if a.group == "fill":
        for ps in PAGE_SIZES:
            emit(fill_point(torch, E, ops, ps, a.reps))
    elif a.group == "ragged":
        ragged_points(torch, E, ops, a.reps, emit)
    else:
        single_points(torch, E, ops, a.group == "fp8", a.reps, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_kvcache_bench.json"))
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
            raise SystemExit(f"prefill_kvcache_bench: {group} did not finish in {CHILD_TIMEOUT_S} s; stopping")
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
            raise SystemExit(f"prefill_kvcache_bench: {group} failed with exit status {r.returncode}; stopping")

    def margin(r):
        return max(r["same_box_noise"], r["new_spread"], r["old_spread"])

    def key(r):
        return [r.get(k) for k in ("point", "fp8", "form", "chunk", "history", "page_size") if r.get(k) is not None]
    by = {g: [r for r in rows if r["goal"] == g] for g in "abc"}
    summary = dict(
        points=len(rows), groups=a.only, same_box_noise_max=max((r["same_box_noise"] for r in rows), default=None),
        a_no_slower_than_the_host_length_kernel=dict(
            same_bits=all(r["same_bits"] for r in by["a"]), ratio_min=min((r["new_over_old"] for r in by["a"]), default=None),
            ratio_max=max((r["new_over_old"] for r in by["a"]), default=None),
            misses=[key(r) + [r["new_over_old"], round(margin(r), 4)] for r in by["a"] if r["new_over_old"] > 1.0 + margin(r)]),
        b_faster_than_the_pieces=dict(
            same_pools=all(r["same_pools"] for r in by["b"]),
            ratios={str(r["page_size"]): r["new_over_old"] for r in by["b"]},
            misses=[key(r) + [r["new_over_old"], round(margin(r), 4)] for r in by["b"] if r["new_over_old"] >= 1.0 - margin(r)]),
        c_no_slower_than_the_sum=dict(
            ratios={r["form"]: r["new_over_old"] for r in by["c"]},
            misses=[key(r) + [r["new_over_old"], round(margin(r), 4)] for r in by["c"] if r["new_over_old"] > 1.0 + margin(r)]))
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, Hkv=HKV, Dh=DH, dtype="bfloat16"), summary=summary, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
