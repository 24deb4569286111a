"""Speculative decoding's token-level launches, on the MI355X.  V = 128256 (Llama-3), bf16 logits; B = 1, 8, 64 slots; kmax = 4, so a step has
T = 5 B rows; two modes: greedy (temperature 0) and topk_topp (temperature 0.7, top-p 0.95, top-k 50).

Goals (set before anything was measured):
  (a) ops.spec_verify on the T rows is no slower, beyond the margin, than ops.sample_logits on the same [T, V] logits (parameters replicated per
      row): it is the same row routine, and the owner search is a handful of cached loads.
  (b) ops.sample_logits of this build is no slower, beyond the margin, than that of the build before the row routine moved into its header
      (--parent-lib: that build's libawq_cdna4.so).  Two builds cannot live in one process, so here the PROCESSES alternate.
Published without a goal: the draft (Lh = 8192), pack and accept launches, the whole draft -> pack -> verify -> accept chain, and the tokens per
slot and step of the toy loop of tests/spec_oracle.py (not a claim about real text).

Method of tools/sample_bench.py: the paths alternate, a figure is the best of `reps` measurements and carries the spread of its measurements,
the relative difference of two measurements of the same thing is the same-box noise, and the margin a ratio is read against is the largest of
the noise and the spreads.  Every figure is device events around one replay of N captured calls, divided by N.

The measurements run in child processes under a time limit.

  python tools/spec_bench.py [--out profiles/spec_bench.json] [--reps 5] [--batches 1,8,64] [--parent-lib PATH]
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

V, KMAX, LH = 128256, 4, 8192
MODES = {"greedy": dict(t=0.0, p=1.0, k=0), "topk_topp": dict(t=0.7, p=0.95, k=50)}
CHILD_TIMEOUT_S = 420


def _figures(torch, fns, n, reps):
    """fns: name -> a function that issues the N calls of one graph.  -> best-of-reps microseconds per call and the spreads, alternating"""
    from kvcache_attn_bench import graph_of, replay_us
    graphs = {name: graph_of(torch, fn) for name, fn in fns.items()}
    times = {name: [] for name in graphs}
    for _ in range(reps):
        for name, g in graphs.items():
            times[name].append(replay_us(torch, g) / n)
    row = {}
    for name, t in times.items():
        row[name + "_us"] = round(min(t), 3)
        row[name + "_spread"] = round((max(t) - min(t)) / min(t), 4)
    return row


def _params(torch, n, m, dev):
    f = dict(dtype=torch.float32, device=dev)
    return dict(temperature=torch.full((n,), m["t"], **f), top_p=torch.full((n,), m["p"], **f),
                top_k=torch.full((n,), m["k"], dtype=torch.int32, device=dev))


def point(torch, ops, B, mode, reps, dev):
    """goal (a) and the unjudged launches at one (B, mode)"""
    m = MODES[mode]
    T = B * (KMAX + 1)
    gen = torch.Generator(device=dev).manual_seed(B)
    logits = (torch.randn(T, V, device=dev, generator=gen) * 3.5).to(torch.bfloat16)
    u = torch.rand(T, device=dev, generator=gen)
    i32 = dict(dtype=torch.int32, device=dev)
    cu = (torch.arange(B + 1, device=dev) * (KMAX + 1)).to(torch.int32)
    # a periodic history: every slot drafts kmax tokens, and greedy verification of random logits rejects them -- the launches' costs do not
    # depend on what is accepted
    history = (torch.arange(LH, device=dev) % 7).to(torch.int32).repeat(B, 1).contiguous()
    hist_len, seqlens = torch.full((B,), LH - 64, **i32), torch.full((B,), 1000, **i32)
    state0 = (hist_len.clone(), seqlens.clone())
    last = torch.full((B,), 3, **i32)
    drafts, draft_len = torch.empty(B, KMAX, **i32), torch.empty(B, **i32)
    cu_out, ids = torch.empty(B + 1, **i32), torch.empty(T, **i32)
    rt = torch.empty(T, **i32)
    out, num, last_out = torch.empty(B, KMAX + 1, **i32), torch.empty(B, **i32), torch.empty(B, **i32)
    slot_kw, row_kw = _params(torch, B, m, dev), _params(torch, T, m, dev)
    n = 50 if B <= 8 else 12

    def draft():
        ops.spec_draft_ngram(history, hist_len, seqlens, vocab=V, kmax=KMAX, ngram_min=1, ngram_max=3, max_len=1 << 20, drafts=drafts, draft_len=draft_len)

    def pack():
        ops.spec_pack(last, drafts, draft_len, seqlens, T, cu_seqlens_q=cu_out, input_ids=ids)

    def verify():
        ops.spec_verify(logits, u, cu_out, ids, row_tokens=rt, **slot_kw)

    def accept():
        ops.spec_accept(rt, ids, cu_out, KMAX, history=history, hist_len=hist_len, seqlens=seqlens, max_len=1 << 20, append=True, advance=True,
                        out_tokens=out, num_emitted=num, last_tokens=last_out)

    def reset():
        hist_len.copy_(state0[0])
        seqlens.copy_(state0[1])

    def chain():
        draft(), pack(), verify(), accept()

    draft(), pack()
    keep = []

    def times(fn):
        def run():
            keep.clear()
            for _ in range(n):
                keep.append(fn())
        return run
    fns = {"verify": times(lambda: ops.spec_verify(logits, u, cu, ids, row_tokens=rt, **slot_kw)),
           "sample": times(lambda: ops.sample_logits(logits, u, **row_kw)),
           "verify_again": times(lambda: ops.spec_verify(logits, u, cu, ids, row_tokens=rt, **slot_kw))}
    row = dict(batch=B, rows=T, mode=mode, vocab=V, calls_per_graph=n)
    row.update(_figures(torch, fns, n, reps))
    row["same_box_noise"] = round(abs(row["verify_us"] - row["verify_again_us"]) / min(row["verify_us"], row["verify_again_us"]), 4)
    row["margin"] = max(row["same_box_noise"], row["verify_spread"], row["sample_spread"], row["verify_again_spread"])
    row["verify_over_sample"] = round(row["verify_us"] / row["sample_us"], 4)
    if mode == "greedy":   # the three small launches do not depend on the sampler's mode
        reset()
        small = _figures(torch, {"draft": times(draft), "pack": times(lambda: (draft(), pack())), "accept": times(lambda: (reset(), accept()))}, n, reps)
        small["pack_us"] = round(small["pack_us"] - small["draft_us"], 3)         # (pack rewrites draft_len: measured behind a draft)
        row.update({k: v for k, v in small.items()})
        row["accept_note"] = "accept_us includes two 4 B device copies that put the lengths back"
    reset()
    row.update(_figures(torch, {"chain": times(lambda: (reset(), chain()))}, n, reps))
    del keep
    torch.cuda.empty_cache()
    return row


def child_points(a):
    import torch

    from llm_awq_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("spec_bench needs the GPU: there is no CPU timing of a GPU kernel")
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            for mode in MODES:
                print("ROW " + json.dumps(point(torch, ops, B, mode, a.reps, "cuda:0")), flush=True)


def child_sample(a):
    """goal (b): awq_sample_logits of the library --lib names, one figure per point (the best of 3 replays).  The entry is bound directly: the
    older build has no awq_spec_* symbols, so llm_awq_amd._capi cannot load it."""
    import ctypes

    import torch

    from llm_awq_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("spec_bench needs the GPU: there is no CPU timing of a GPU kernel")
    dev = "cuda:0"
    fn = ctypes.CDLL(a.lib).awq_sample_logits
    fn.restype, fn.argtypes = _capi.SIGNATURES["awq_sample_logits"]

    def sample_logits(logits, u, tokens, temperature, top_p, top_k):
        st = fn(logits.data_ptr(), _capi.AWQ_BF16, logits.shape[0], logits.shape[1], u.data_ptr(), temperature.data_ptr(), top_k.data_ptr(),
                top_p.data_ptr(), None, None, None, 0, None, None, 0, None, 0, 0, tokens.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            for mode, m in MODES.items():
                gen = torch.Generator(device=dev).manual_seed(B)
                logits = (torch.randn(B, V, device=dev, generator=gen) * 3.5).to(torch.bfloat16)
                u = torch.rand(B, device=dev, generator=gen)
                kw = _params(torch, B, m, dev)
                n = 100 if B <= 8 else 30
                tokens = torch.empty(B, dtype=torch.int32, device=dev)

                def run():
                    for _ in range(n):
                        sample_logits(logits, u, tokens, **kw)
                fig = _figures(torch, {"sample": run}, n, 3)
                print("ROW " + json.dumps(dict(batch=B, mode=mode, sample_us=fig["sample_us"])), flush=True)


def run_child(args):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"spec_bench: the measurements did not finish in {CHILD_TIMEOUT_S} s; stopping")
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + "\n" + r.stderr[-4000:] + "\n")
        raise SystemExit(f"spec_bench: the measurements failed with exit status {r.returncode}; stopping")
    return [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]


def toy_tokens_per_step():
    from tests import spec_oracle as S
    s = S.toy_state(0)
    _, num, _, steps = S.spec_loop(s)
    took = (num > 0).sum(0)
    return dict(tokens=num.sum(0).tolist(), slot_steps=took.tolist(), tokens_per_slot_step=[round(float(t) / float(k), 3) for t, k in zip(num.sum(0), took)],
                steps=int(steps), serial_steps=int(S.serial_loop(s)[2]), kmax=S.TOY_KMAX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--parent-lib", default=None, help="libawq_cdna4.so of the build before this change (goal b)")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, choices=["points", "sample"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_points(a) if a.child == "points" else child_sample(a)
    common = ["--reps", str(a.reps), "--batches", a.batches]
    rows = run_child(["--child", "points"] + common)
    for r in rows:
        print(json.dumps(r), flush=True)
    summary = dict(points=len(rows),
                   goal_a_verify_no_slower_than_sample_beyond_margin=all(r["verify_over_sample"] <= 1.0 + r["margin"] for r in rows),
                   verify_over_sample={f'{r["batch"]}/{r["mode"]}': r["verify_over_sample"] for r in rows},
                   margin={f'{r["batch"]}/{r["mode"]}': r["margin"] for r in rows},
                   toy_loop=toy_tokens_per_step())
    ab = None
    if a.parent_lib:
        from llm_awq_amd._capi import LIB_PATH
        builds = {"this": LIB_PATH, "parent": os.path.abspath(a.parent_lib), "this_again": LIB_PATH}
        times = {name: {} for name in builds}
        for _ in range(a.reps):   # the processes alternate
            for name, lib in builds.items():
                for r in run_child(["--child", "sample", "--lib", lib] + common):
                    times[name].setdefault(f'{r["batch"]}/{r["mode"]}', []).append(r["sample_us"])
        ab = {}
        for key in times["this"]:
            best = {name: min(times[name][key]) for name in builds}
            spread = {name: (max(times[name][key]) - best[name]) / best[name] for name in builds}
            noise = abs(best["this"] - best["this_again"]) / min(best["this"], best["this_again"])
            ab[key] = dict(this_us=best["this"], parent_us=best["parent"], this_again_us=best["this_again"], this_over_parent=round(best["this"] / best["parent"], 4),
                           margin=round(max(noise, *spread.values()), 4))
        summary["goal_b_sample_logits_no_slower_than_parent_beyond_margin"] = all(v["this_over_parent"] <= 1.0 + v["margin"] for v in ab.values())
    else:
        summary["goal_b_sample_logits_no_slower_than_parent_beyond_margin"] = "not measured (no --parent-lib)"
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(V=V, dtype="bfloat16", kmax=KMAX, draft_history=LH, modes=MODES), summary=summary, rows=rows, sample_logits_ab=ab), f,
                      indent=1)


if __name__ == "__main__":
    main()
