"""Return codes of the six dense W4 cdna4 linear entries of the C ABI under single and paired argument faults (host only).

    python -m tools.linear_entry_codes            # print a summary of what the built library answers
    python -m tools.linear_entry_codes --write    # (re)generate tests/linear_entry_codes.json from the built library

Same scheme as tools/kv_entry_codes.py: each entry starts from one valid argument set per row-count class over fake aligned pointers
(nothing is dereferenced: every recorded case is refused by the entry's own checks), `cases(entry)` applies every single fault and every
pair of faults from two different check phases.  The entries test bias and sz_half alignment in some row-count classes only and let a
misaligned sz_half silently take the sz_packed path: a fault an entry accepts would reach a launch, so the generator hides every device
from the process, records such a case as null and tests/test_linear_entry_codes_host.py skips it.

The committed table was recorded from the commit BEFORE the entries were moved onto linear_route (csrc/awq_linear_route.hpp); it is
replayed, never regenerated together with a change to the entries.
"""
from __future__ import annotations

import itertools
import json
import os
import sys

from tools.kv_entry_codes import P16, ids_digest, param_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "linear_entry_codes.json")
AWQ_ERR_LAUNCH = -8
ENTRIES = ["awq_w4a16_forward_cdna4", "awq_w4a16_forward_cdna4_szh", "awq_w4a16_gemm_cdna4", "awq_w4a16_gemv_cdna4",
           "awq_w4a16_mlp_gate_up_forward_cdna4_ws", "awq_w4a16_partial_cdna4"]
# one row count per class of the routes: decode, 9 .. 16, skinny, mid-M (by shape and 65 .. 128), masked tile, skinny above 128 rows, tiles
ROWS = [1, 8, 9, 16, 17, 40, 64, 100, 160, 255, 256, 300]
N, K = 8192, 8192   # (n = 8192: the mid-M kernel also takes 33 .. 64 rows)
INTS = {"m": [0, -1], "n": [0, 8, 4100, 4104], "n2": [0, 8, 4100, 4104, 4112], "k": [0, 64, 4000], "group_size": [64], "dtype": [2, -1]}


def base_args(entry: str, m: int) -> dict:
    a = {}
    for n in param_names(entry):
        a[n] = {"m": m, "n": N, "n2": N, "k": K, "group_size": 128, "dtype": 1, "workspace": 0, "workspace_bytes": 0, "stream": 0}.get(n, P16)
    return a


def faults(entry: str, m: int) -> list[tuple[str, str, dict]]:
    out = []
    for n, v in base_args(entry, m).items():
        if n in ("stream", "workspace_bytes"):
            continue
        if n == "workspace":
            out += [("workspace=+4", "tail", {"workspace": P16 + 4, "workspace_bytes": 1 << 30}), ("workspace=small", "tail", {"workspace": P16, "workspace_bytes": 16})]
        elif v == P16:
            out += [(f"{n}=null", "null", {n: 0}), (f"{n}=+2", "align", {n: P16 + 2}), (f"{n}=+8", "align", {n: P16 + 8})]
        else:
            out += [(f"{n}={x}", "dtype" if n == "dtype" else ("group" if n == "group_size" else "shape"), {n: x}) for x in INTS[n]]
    if entry.endswith("gemv_cdna4"):
        out.append(("m=17", "shape", {"m": 17}))
    return out


def cases(entry: str) -> list[tuple[str, dict]]:
    out = []
    for m in ROWS:
        if entry.endswith("gemv_cdna4") and m > 16:
            continue
        a, fs = base_args(entry, m), faults(entry, m)
        out += [(f"m{m}: {i}", {**a, **d}) for i, _, d in fs]
        for (i0, p0, d0), (i1, p1, d1) in itertools.combinations(fs, 2):
            if p0 != p1 and not set(d0) & set(d1):
                out.append((f"m{m}: {i0} & {i1}", {**a, **d0, **d1}))
    return out


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
        print(f"{e}: {len(cs)} cases, { {c: kept.count(c) for c in sorted(set(kept), key=str)} }")
    if "--write" in sys.argv:
        import subprocess
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        with open(TABLE, "w") as f:
            json.dump({"generated_from": head, "entries": table}, f, separators=(",", ":"))
            f.write("\n")
        print("wrote", TABLE, sum(len(t["codes"]) for t in table.values()), "codes")


if __name__ == "__main__":
    main()
