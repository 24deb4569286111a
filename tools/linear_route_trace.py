"""Proof that a change to the routing of the dense W4 cdna4 linear entries moved no call to another kernel: one fixed sequence of about 300
real calls through the six entries (every leaf of csrc/awq_linear_route.hpp, every knob block of tests/linear_route_cases.py), to be run
under a kernel trace on two builds of the library and compared launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python -m tools.linear_route_trace run OUT/calls.json    # on each build, same machine
    python -m tools.linear_route_trace compare A/calls.json A_trace.csv B/calls.json B_trace.csv                             # anywhere; exit 1 on any difference

`run` issues the calls one after the other on the null stream through ctypes, over zero-filled device buffers sized for the largest call,
with a synchronise and one marker kernel (a torch in-place add) between calls; it writes each call's description and -- where the library
has awq_w4a16_linear_route_cdna4 -- its route words.  `compare` splits both traces at the markers and demands, call by call, the same
kernel names (template arguments included), grids, blocks and LDS sizes; where a build recorded route words it also checks that the kernels
traced for a call belong to the family of its leaf (LEAF_KERNELS) and that a bias-add launch follows exactly where the route says so.
"""
from __future__ import annotations

import csv
import json
import os
import re
import sys

ENTRIES = ["forward", "forward_szh", "gemm", "gemv", "gate_up", "partial"]
SZP, SZH, BIAS, WS, WS_TILES = 1, 2, 4, 8, 16
ROWS = [1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 71, 72, 128, 129, 192, 255, 256, 300, 2048]
O, DOWN, QKV, PAIR = (4096, 4096), (4096, 14336), (6144, 4096), (28672, 4096)
DEFAULTS = dict(midm=1, midm_min=65, midm_max=128, gemm_small_m=1, gemm_variant=0, mlp_skinny_max=64, skinny16_szh=1, gemv_dma=1)
LEAF_KERNELS = {1: ("gemv_dma_kernel", "gemv_dma_kernel_m1", "skinny_cdna4_kernel"), 2: ("gemv_cdna4_kernel",), 3: ("midm_kernel",), 4: ("skinny_cdna4_kernel",),
                5: ("skinny_cdna4_kernel", "skinny_splitk_kernel"), 6: ("skinny_cdna4_kernel",),
                7: ("gemm_cdna4_v6_kernel", "gemm_cdna4_v6_pair_kernel", "gemm_cdna4_v4n_kernel", "splitk_reduce_kernel"),
                8: ("gemv_w4a16_kernel", "gemm_w4a16_128x128_kernel", "gemm_w4a16_256x256_kernel", "gemm_cdna4_v6_kernel", "gemm_cdna4_v6_pair_kernel",
                    "gemm_cdna4_v4n_kernel", "splitk_reduce_kernel")}


def calls():
    """(knobs, entry, m, n, k, flags): the fixed sequence."""
    out = []

    def add(knobs, entry, ms, shapes, flag_sets):
        out.extend((knobs, ENTRIES.index(entry), m, n, k, f) for (n, k) in shapes for f in flag_sets for m in ms)

    d = {}
    add(d, "forward", ROWS, [O, DOWN], [SZP | BIAS | WS])
    add(d, "forward", [17, 64, 160], [PAIR], [SZP | BIAS | WS])
    add(d, "forward", [16, 40, 64], [(8192, 8192), (8192, 28672)], [SZP | BIAS | WS])
    add(d, "forward", [1, 12, 40, 300], [(3072, 768)], [BIAS, 0])
    add(d, "forward", [8, 64, 100, 255, 256, 2048], [QKV], [SZP | WS])
    add(d, "forward", [40, 100, 300], [O], [SZP | BIAS])
    add(d, "forward_szh", [1, 9, 16, 17, 64, 100, 160, 256, 2048], [O, PAIR], [SZP | SZH | BIAS | WS])
    add(d, "forward_szh", [12, 100, 300], [(3072, 768)], [SZH | BIAS, SZP | SZH])
    add(d, "gemm", [1, 8, 9, 64, 65, 128, 200, 256, 1024], [O, DOWN], [SZP | WS])
    add(d, "gemm", [4, 12, 40, 300], [(768, 3072)], [0])
    add(d, "gemv", [1, 4, 8, 9, 16], [O], [SZP, 0])
    add(d, "gate_up", [1, 4, 8, 9, 16, 17, 48, 49, 64, 65, 128, 129, 255, 256, 2048], [PAIR], [SZP, SZP | SZH | WS | WS_TILES])
    add(d, "gate_up", [12, 100, 300, 2048], [PAIR], [SZP | SZH, SZP | WS])   # (a workspace below the tile kernels' size: dropped by their row only)
    add(d, "gate_up", [1, 2, 9, 49, 64], [(57344, 8192), (22016, 4096)], [SZP | SZH])
    add(d, "partial", [1, 5, 8, 9, 16, 40, 64, 100, 200, 256, 512], [DOWN], [SZP, SZP | SZH])
    add(d, "partial", [4, 16, 64], [(8192, 28672)], [SZP])
    k = dict(midm=0)
    add(k, "forward", [9, 40, 64, 100, 128, 200], [O, DOWN], [SZP | BIAS | WS])
    add(k, "gate_up", [16, 40, 64, 100], [PAIR], [SZP, SZP | SZH])
    add(k, "partial", [40, 100], [DOWN], [SZP])
    add(k, "forward_szh", [12, 100], [O], [SZP | SZH | BIAS | WS])
    k = dict(midm_min=9, midm_max=255)
    add(k, "forward", [9, 64, 129, 192, 255], [O], [SZP | BIAS | WS])
    add(k, "forward", [160, 200], [PAIR], [SZP | WS])
    add(k, "gate_up", [12, 200], [PAIR], [SZP | SZH])
    k = dict(midm_max=192)
    add(k, "forward", [150, 192, 193], [O], [SZP | BIAS | WS])
    add(k, "forward", [160], [PAIR], [SZP | WS])
    add(dict(gemm_small_m=0), "forward", [129, 200, 255], [O, PAIR], [SZP | BIAS | WS])
    add(dict(gemm_small_m=2), "forward", [9, 40, 129], [O], [SZP | BIAS | WS])
    for v in (1, 2, 3, 4, 5):
        k = dict(gemm_variant=v)
        add(k, "forward", [1, 12, 40, 100, 300], [(3072, 768)], [SZP | BIAS | WS])
        add(k, "forward_szh", [100], [(3072, 768)], [SZP | SZH | BIAS | WS])
        add(k, "partial", [100], [(3072, 768)], [SZP])
    add(dict(midm=0, mlp_skinny_max=8), "gate_up", [9, 16, 40, 64], [PAIR], [SZP, SZP | SZH])
    k = dict(skinny16_szh=0)
    add(k, "forward_szh", [12], [O], [SZP | SZH | BIAS | WS])
    add(k, "gate_up", [12], [PAIR], [SZP | SZH])
    k = dict(gemv_dma=0)
    add(k, "forward", [1, 8], [O], [SZP | BIAS | WS])
    add(k, "gemv", [4], [O], [SZP])
    return out


def run(calls_path: str) -> None:
    import ctypes

    import torch

    from llm_awq_amd import _capi

    L, cs = _capi.lib(), calls()
    has_query = hasattr(ctypes.CDLL(_capi.LIB_PATH), "awq_w4a16_linear_route_cdna4")
    ws_q = {0: L.awq_w4a16_forward_cdna4_workspace_bytes, 4: L.awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes}
    need = dict(x=0, qw=0, sc=0, sz=0, bias=0, out=0, ws=1 << 20)
    for _, e, m, n, k, f in cs:   # every buffer is sized for the largest call that reads or writes it
        for key, b in dict(x=m * k * 2, qw=n * k // 2, sc=n * (k // 128) * 2, sz=n * (k // 128) * 4, bias=n * 2, out=m * n * 4).items():
            need[key] = max(need[key], b)
        need["ws"] = max(need["ws"], ws_q[0](m, n, k), ws_q[4](m, n, k))
    buf = {key: torch.zeros(b + 256, dtype=torch.uint8, device="cuda") for key, b in need.items()}
    zeros2, szh = torch.zeros_like(buf["sc"]), torch.zeros_like(buf["sz"])
    p = {key: t.data_ptr() for key, t in buf.items()}
    assert all(v % 64 == 0 for v in p.values())
    mark = torch.zeros(64, device="cuda")
    log, knobs_now = [], None
    for knobs, e, m, n, k, f in cs:
        if knobs != knobs_now:
            _capi.tune(**{**DEFAULTS, **knobs})
            knobs_now = knobs
        sz_packed, sz_half, bias = (p["sz"] if f & SZP else None), (szh.data_ptr() if f & SZH else None), (p["bias"] if f & BIAS else None)
        ws, ws_bytes = (p["ws"], need["ws"] if (e != 4 or f & WS_TILES) else 16) if f & WS else (None, 0)
        torch.cuda.synchronize()
        mark.add_(1.0)   # the marker between calls
        if e == 0:
            rc = L.awq_w4a16_forward_cdna4(p["x"], p["qw"], p["sc"], zeros2.data_ptr(), sz_packed, bias, p["out"], m, n, k, 128, 1, ws, ws_bytes, None)
        elif e == 1:
            rc = L.awq_w4a16_forward_cdna4_szh(p["x"], p["qw"], p["sc"], zeros2.data_ptr(), sz_packed, sz_half, bias, p["out"], m, n, k, 128, 1, ws, ws_bytes, None)
        elif e == 2:
            rc = L.awq_w4a16_gemm_cdna4(p["x"], p["qw"], p["sc"], zeros2.data_ptr(), sz_packed, p["out"], m, n, k, 128, 1, ws, ws_bytes, None)
        elif e == 3:
            rc = L.awq_w4a16_gemv_cdna4(p["x"], p["qw"], p["sc"], zeros2.data_ptr(), sz_packed, p["out"], m, n, k, 128, 1, None)
        elif e == 4:
            rc = L.awq_w4a16_mlp_gate_up_forward_cdna4_ws(p["x"], p["qw"], sz_packed, sz_half, p["out"], m, n, k, 128, 1, ws, ws_bytes, None)
        else:
            rc = L.awq_w4a16_partial_cdna4(p["x"], p["qw"], sz_packed, sz_half, p["out"], m, n, k, 128, 1, None)
        torch.cuda.synchronize()
        assert rc == 0, (rc, knobs, ENTRIES[e], m, n, k, f)
        words = None
        if has_query:
            o = (ctypes.c_int * 8)()
            assert L.awq_w4a16_linear_route_cdna4(e, m, n, k, f, o) == o[0] > 0
            words = list(o)
        log.append(dict(knobs=knobs, entry=ENTRIES[e], m=m, n=n, k=k, flags=f, route=words))
        print(ENTRIES[e], m, n, k, f, knobs, words, flush=True)
    _capi.tune(**DEFAULTS)
    mark.add_(1.0)
    torch.cuda.synchronize()
    with open(calls_path, "w") as fh:
        json.dump(log, fh)
    print("calls:", len(log))


def listing(calls_path: str, trace_csv: str):
    """per call: [(kernel name, grid, block, LDS bytes), ...]"""
    log = json.load(open(calls_path))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "awq::" not in name:   # a marker (or the buffers' fills before the first call): the next call starts
            if cur is None or cur:
                cur = []
                groups.append(cur)
            continue
        cur.append((name, tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"])))
    groups = [g for g in groups if g]
    assert len(groups) == len(log), (len(groups), len(log))
    return log, groups


def compare(a_calls, a_csv, b_calls, b_csv) -> int:
    (la, ga), (lb, gb) = listing(a_calls, a_csv), listing(b_calls, b_csv)
    strip = lambda l: [{k: v for k, v in c.items() if k != "route"} for c in l]
    assert strip(la) == strip(lb), "the two runs issued different calls"
    diffs = [(i, la[i], ga[i], gb[i]) for i in range(len(la)) if ga[i] != gb[i]]
    print(f"A: {len(la)} calls, {sum(map(len, ga))} kernel launches; B: {len(lb)} calls, {sum(map(len, gb))} kernel launches; {len(diffs)} calls differ")
    for i, c, x, y in diffs:
        print(f"call {i} {c}:\n  A {x}\n  B {y}")
    wrong = 0
    for log, groups, tag in ((la, ga, "A"), (lb, gb, "B")):
        routed = [(c, g) for c, g in zip(log, groups) if c["route"]]
        for c, g in routed:
            fam = [re.match(r"(?:void )?(?:awq::)?(?:\(anonymous namespace\)::)?(\w+)", name).group(1) for name, *_ in g]
            body, tail = (fam[:-1], fam[-1:]) if c["route"][3] == 2 else (fam, [])
            if not body or any(f not in LEAF_KERNELS[c["route"][0]] for f in body) or tail != (["bias_add_kernel"] if c["route"][3] == 2 else []):
                wrong += 1
                print(f"{tag}: {c} ran {fam}: not the family of its leaf")
        if routed:
            leaves, rows_ = sorted({c["route"][0] for c, _ in routed}), len({(c["entry"], c["route"][6]) for c, _ in routed})
            print(f"{tag}: {len(routed)} routed calls checked against their leaf's kernel family; leaves seen {leaves}; {rows_} distinct (entry, row) pairs; {wrong} wrong")
    return 1 if diffs or wrong else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        run(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:6]))
