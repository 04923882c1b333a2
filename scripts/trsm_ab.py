#!/usr/bin/env python3
"""A/B of the triangular solve's schedules (smfv_trsm_plan_*, TrsmPlan).

    python scripts/trsm_ab.py [--matrix stencil|irregular] [--thin 16,256,1024] [--rounds 3]

Lower triangle of a cop20k_A stand-in (stencil) or cop20k_irregular_surrogate
with its diagonal made dominant (so the solution stays finite), K = 32.  Forms,
timed with bench.py's discipline as scripts/transpose_ab.py does (copies of
(plans, X, Y) rotated; the launches of `steps` solves captured into one
hipGraph on a side stream; a replay timed with device events after untimed
stabilising replays), the forms alternating within each round:

  auto      chain="auto": thin runs in the one-block kernel, wide levels as grids
  off       chain="off":  one launch per level
  all       chain="all":  every level in the one-block kernel, one launch
  thinN     chain="auto" with the thin-level threshold at N rows
  spmm      A X of the same pattern (the whole matrix), for scale

A form's `steps` is chosen so that its graph holds about --nodes kernel nodes.
Before anything is timed every form is compared bit for bit with `auto`, and
`auto` with the numpy substitution loop on the first --check-rows rows.  Prints
one JSON line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STABILIZE_S = 0.1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("stencil", "irregular"), default="stencil")
    ap.add_argument("--thin", default="16,256,1024", help="thresholds tried beside the default (rows)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=6000, help="kernel nodes per captured graph, about")
    ap.add_argument("--max-steps", type=int, default=40)
    ap.add_argument("--cold-bytes", type=float, default=1.0e9)
    ap.add_argument("--check-rows", type=int, default=4000)
    args = ap.parse_args()

    import numpy as np
    import torch

    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import inputs

    if not torch.cuda.is_available():
        raise SystemExit("trsm_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K = 32
    A = inputs.cop20k_surrogate() if args.matrix == "stencil" else inputs.cop20k_irregular_surrogate()
    m, nnz = A.numRows, A.nnz
    rp, ci = np.asarray(A.rowPtr, np.int64), np.asarray(A.colIndices, np.int64)
    r = np.repeat(np.arange(m), np.diff(rp))
    va = np.array(A.values, np.float64)
    low = ci < r
    va[ci == r] = 1.0 + np.bincount(r[low], np.abs(va[low]), minlength=m)[r[ci == r]]
    A = inputs.SparseMatrix(values=va, colIndices=A.colIndices, rowPtr=A.rowPtr, numRows=m, numCols=A.numCols)
    X = inputs.generateLargeFatVector(m, K)

    forms = {"auto": {}, "off": {"chain": "off"}, "all": {"chain": "all"}}
    for t in (int(v) for v in args.thin.split(",") if v):
        forms[f"thin{t}"] = {"thin_rows": t}
    host = {f: smfv.trsm_analyse(A, K, "lower", **kw) for f, kw in forms.items()}
    strict = host["auto"]["strict_entries"]
    model = {"plan_stream": 12 * strict + 16 * m, "x_and_y": 16 * m * K, "y_gathered": 8 * K * strict,
             "spmm": 12 * nnz + 4 * (m + 1) + 16 * m * K}
    ncopies = max(1, min(12, math.ceil(args.cold_bytes / (model["plan_stream"] + model["x_and_y"])) + 1))

    copies = []
    for _ in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        c = {f: smfv.TrsmPlan(dA, K, "lower", **kw) for f, kw in forms.items()}
        c["spmm"] = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K)
        c["X"] = torch.from_numpy(X).to(dev)
        c["Y"] = torch.empty((m, K), dtype=torch.float64, device=dev)
        copies.append(c)
    c0 = copies[0]
    stats = {f: c0[f].stats() for f in forms}

    # widths of the levels (host), as a histogram over powers of two
    lev = np.zeros(m, np.int32)
    import ctypes
    from sparsematrixmultiplicationmpi_amd._lib import call
    ip = ctypes.POINTER(ctypes.c_int)
    order, nlev = np.zeros(m, np.int32), ctypes.c_int(0)
    call("smfv_trsm_levels", m, np.ascontiguousarray(A.rowPtr, np.int32).ctypes.data_as(ip),
         np.ascontiguousarray(A.colIndices, np.int32).ctypes.data_as(ip), 0, lev.ctypes.data_as(ip),
         order.ctypes.data_as(ip), ctypes.byref(nlev))
    w = np.bincount(lev)[1:]
    edges = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 1 << 30]
    hist = {f"{edges[i]}-{edges[i + 1] - 1}" if i + 2 < len(edges) else f">={edges[i]}": int(n)
            for i, n in enumerate(np.histogram(w, bins=edges)[0])}

    # every form against auto, auto against the substitution loop on the first rows
    ref = c0["auto"].solve(c0["X"]).clone()
    torch.cuda.synchronize()
    agree = {}
    for f in forms:
        Y = c0[f].solve(c0["X"])
        torch.cuda.synchronize()
        agree[f] = bool(torch.equal(Y.view(torch.int64), ref.view(torch.int64)))
    n_chk = min(args.check_rows, m)
    Yh = np.empty((n_chk, K))
    civ, rpv = np.asarray(A.colIndices), np.asarray(A.rowPtr)
    for i in range(n_chk):
        s, d = X[i].copy(), None
        for j in range(int(rpv[i]), int(rpv[i + 1])):
            cc = civ[j]
            if cc < i:
                p = va[j] * Yh[cc]
                s = s - p
            elif cc == i:
                d = va[j] if d is None else d + va[j]
        Yh[i] = s / d
    got = ref[:n_chk].cpu().numpy()
    check = bool(np.array_equal(got.view(np.uint64), Yh.view(np.uint64))) and bool(np.isfinite(ref.cpu().numpy()).all())

    def step(form: str, i: int) -> None:
        c = copies[i % ncopies]
        if form == "spmm":
            c["spmm"].run(c["X"], c["Y"])
        else:
            c[form].solve(c["X"], c["Y"])

    names = list(forms) + ["spmm"]
    steps = {f: max(2, min(args.max_steps, args.nodes // max(1, stats[f]["launches"]))) for f in forms}
    steps["spmm"] = 200
    graphs = {}
    for form in names:
        for i in range(max(2, ncopies)):
            step(form, i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(steps[form]):
                    step(form, i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[form] = g

    def timed(form: str) -> float:
        g = graphs[form]
        t_end = time.time() + STABILIZE_S
        while time.time() < t_end:
            g.replay()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps[form]  # us per solve

    us = {form: [] for form in names}
    for _ in range(args.rounds):
        for form in names:
            us[form].append(round(timed(form), 2))
    med = {form: statistics.median(v) for form, v in us.items()}
    keys = ("levels", "widest_level", "launches", "chain_launches", "chain_rows", "chain_max_levels", "thin_rows",
            "plan_bytes", "analysis_ms")
    print(json.dumps({
        "what": f"T Y = X, lower triangle of the cop20k {args.matrix} stand-in, K = 32, us per solve (copies rotated)",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "copies_rotated": ncopies, "m": m, "nnz": nnz,
        "strict_entries": strict, "level_widths": hist, "median_width": float(np.median(w)),
        "steps_per_graph": steps, "us": us, "median_us": med,
        "us_per_level": {f: round(med[f] / max(1, stats[f]["levels"]), 3) for f in forms},
        "model_bytes": model, "plan_stats": {f: {k: stats[f][k] for k in keys} for f in forms}, "host_analysis": host["auto"],
        "forms_bitwise_equal_auto": agree, "auto_bitwise_vs_loop_rows": n_chk, "auto_bitwise_vs_loop": check}))
    if not (check and all(agree.values())):
        raise SystemExit("trsm_ab: the forms disagree, or auto differs from the substitution loop")


if __name__ == "__main__":
    main()
