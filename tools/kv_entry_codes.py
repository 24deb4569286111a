"""Return codes of the twelve natural-KV-cache entries of the C ABI under single and paired argument faults (host only).

    python -m tools.kv_entry_codes            # print a summary of what the built library answers
    python -m tools.kv_entry_codes --write    # (re)generate tests/kv_entry_codes.json from the built library

Each entry starts from one valid argument set over fake aligned pointers (nothing is dereferenced: every recorded case is refused by
the entry's own checks).  `cases(entry)` applies every single fault of the table below and every pair of faults from two different
check phases (null / dtype / shape / align / tail).  Attention entries keep the workspace NULL unless the workspace is the thing
perturbed, so their no-fault case answers AWQ_ERR_WORKSPACE; store entries have no no-fault case.  A fault that an entry accepts (a
4-byte step of an int pointer, an 8-element step of a T-cache stride, Sq * G > 128 on the host-length entries, ...) would reach a launch:
the generator hides every device from the process, records such a case as null and tests/test_kv_entry_codes_host.py skips it.

The committed table pins the behaviour of the entries across refactors of their validation: it is generated once and replayed, never
regenerated together with a change to the checks.
"""
from __future__ import annotations

import ctypes
import hashlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "kv_entry_codes.json")
AWQ_ERR_LAUNCH = -8

STORE_ENTRIES = ["awq_rope_kv_store_natural", "awq_rope_kv_store_natural_fp8", "awq_rope_kv_store_natural_pos",
                 "awq_rope_kv_store_natural_pos_fp8", "awq_rope_kv_store_paged_pos", "awq_rope_kv_store_paged_pos_fp8"]
ATTN_ENTRIES = ["awq_attn_splitkv", "awq_attn_splitkv_kv8", "awq_attn_kvcache", "awq_attn_kvcache_kv8", "awq_attn_kvcache_paged",
                "awq_attn_kvcache_paged_kv8"]
ENTRIES = STORE_ENTRIES + ATTN_ENTRIES

B, BC, S, H, HKV, DH, ROT, LMAX = 2, 3, 3, 8, 2, 128, 64, 4096
SQ, SK = 2, 4096                     # host-length entries: 4096 keys split (the plan's floor is 2048)
PAGE, PPS, NPAGES = 128, 16, 40      # paged entries: a table row names 2048 keys


def param_names(entry: str) -> list[str]:
    text = open(os.path.join(ROOT, "include", "awq_cdna4.h")).read()
    m = re.search(r"^int " + entry + r"\((.*?)\);", text, re.S | re.M)
    return [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]


_buf = (ctypes.c_char * 64)()
P16 = (ctypes.addressof(_buf) + 15) & ~15  # fake pointer, 16-byte aligned, never dereferenced


def base_args(entry: str) -> dict:
    """One valid argument set (attention entries: but for the NULL workspace)."""
    paged, fp8 = "paged" in entry, entry.endswith(("fp8", "kv8"))
    rows = PAGE if paged else (SK if "splitkv" in entry else LMAX)
    kv_row = HKV * DH
    a = {}
    for n in param_names(entry):
        if n in ("workspace", "stream"):
            a[n] = 0
        elif n == "workspace_bytes":
            a[n] = 0
        elif n.endswith("_row_stride"):
            a[n] = {"q": H * DH, "qkv": (H + 2 * HKV) * DH, "k": kv_row, "v": kv_row, "k_scale": HKV, "v_scale": HKV,
                    "table": PPS}[n[:-len("_row_stride")]]
        elif n.endswith(("_batch_stride", "_page_stride")):
            who = n.rsplit("_", 2)[0]
            a[n] = {"q": SQ * H * DH, "qkv": S * (H + 2 * HKV) * DH, "k": rows * kv_row, "v": rows * kv_row, "k_scale": rows * HKV,
                    "v_scale": rows * HKV}[who]
        else:
            a[n] = {"batch": B, "cache_batch": BC, "seqlen": S, "nheads": H, "nheads_kv": HKV, "head_dim": DH, "rot_dim": ROT, "lmax": LMAX,
                    "start_pos": 5, "table_rows": 4096, "seqlen_q": SQ, "seqlen_k": SK, "seqlen_offset": 1,
                    "max_seqlen_k": 1024 if paged else 2048, "num_pages": NPAGES, "page_size": PAGE, "pages_per_seq": PPS,
                    "softmax_scale": 0.088, "causal": 1, "dtype": 1}.get(n, P16)  # everything else is a pointer
    return a


def faults(entry: str) -> list[tuple[str, str, dict]]:
    """(id, phase, {argument: value}) for every single fault of the entry."""
    a, out = base_args(entry), []
    cap = PAGE * PPS if "paged" in entry else LMAX
    ints = {"batch": [0], "cache_batch": [B - 1], "seqlen": [0], "nheads": [0, 7], "nheads_kv": [0, 3], "head_dim": [32, 96, 256],
            "rot_dim": [0, 8, 24, DH + 16], "lmax": [0, 5 + S - 1], "start_pos": [-1, LMAX - S + 1], "table_rows": [0],
            "seqlen_q": [0, 33], "seqlen_k": [0], "num_pages": [0], "page_size": [0, 32, 96], "pages_per_seq": [0]}
    for n, v in a.items():
        if n in ("stream", "workspace_bytes", "softmax_scale", "causal"):
            continue
        if n == "workspace":
            need = workspace_need(entry)
            out += [("workspace=small", "tail", {"workspace": P16, "workspace_bytes": need - 16}),
                    ("workspace=+4", "tail", {"workspace": P16 + 4, "workspace_bytes": need})]
        elif v == P16:
            out += [(f"{n}=null", "null", {n: 0}), (f"{n}=+2", "align", {n: P16 + 2}), (f"{n}=+4", "align", {n: P16 + 4})]
        elif n.endswith("_stride"):
            out.append((f"{n}=neg", "shape", {n: -16}))
            if n.endswith("_row_stride"):
                out.append((f"{n}=small", "shape", {n: v - 16 if v >= 16 else v - 1}))
            out += [(f"{n}=+4", "align", {n: v + 4}), (f"{n}=+8", "align", {n: v + 8})]
        elif n == "dtype":
            out.append(("dtype=2", "dtype", {n: 2}))
        elif n == "max_seqlen_k":
            out += [(f"{n}=0", "shape", {n: 0}), (f"{n}=cap", "tail", {n: cap}), (f"{n}=cap+1", "tail", {n: cap + 1})]
        elif n == "seqlen_offset":
            out.append((f"{n}=-1", "tail", {n: -1}))
        else:
            out += [(f"{n}={x}", "shape", {n: x}) for x in ints[n]]
    return out


def workspace_need(entry: str) -> int:
    from llm_awq_amd import _capi
    a = base_args(entry)
    if "splitkv" in entry:
        return _capi.lib().awq_attn_splitkv_workspace_bytes(B, H, HKV, DH, SQ, SK, 1)
    return _capi.lib().awq_attn_kvcache_workspace_bytes(B, H, HKV, DH, SQ, a["max_seqlen_k"])


def cases(entry: str) -> list[tuple[str, dict]]:
    """(id, arguments) of every case of the entry, in a fixed order."""
    a, fs = base_args(entry), faults(entry)
    out = [("none", dict(a))] if entry in ATTN_ENTRIES else []
    out += [(i, {**a, **d}) for i, _, d in fs]
    for (i0, p0, d0), (i1, p1, d1) in itertools.combinations(fs, 2):
        if p0 != p1 and not set(d0) & set(d1):
            out.append((i0 + " & " + i1, {**a, **d0, **d1}))
    return out


def ids_digest(cs) -> str:
    return hashlib.sha256("\n".join(i for i, _ in cs).encode()).hexdigest()[:16]


def codes(entry: str) -> list[int]:
    from llm_awq_amd import _capi
    fn = getattr(_capi.lib(), entry)
    return [fn(*args.values()) for _, args in cases(entry)]


def main() -> None:
    # no device for this process: a case the entry accepts fails at its launch (AWQ_ERR_LAUNCH) and never runs a kernel over the fake pointers
    os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = ""
    table = {}
    for e in ENTRIES:
        cs, got = cases(e), codes(e)
        kept = [None if c in (0, AWQ_ERR_LAUNCH) else c for c in got]
        table[e] = {"ids": ids_digest(cs), "codes": kept}
        hist = {c: kept.count(c) for c in sorted(set(kept), key=str)}
        print(f"{e}: {len(cs)} cases, {hist}")
    if "--write" in sys.argv:
        import subprocess
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        with open(TABLE, "w") as f:
            json.dump({"generated_from": head, "entries": table}, f, separators=(",", ":"))
            f.write("\n")
        print("wrote", TABLE, sum(len(t["codes"]) for t in table.values()), "codes")


if __name__ == "__main__":
    main()
