#!/usr/bin/env python3
"""A/B of the ILU(0) schedules (smfv_ilu0_plan_*, Ilu0Plan).

    python scripts/ilu0_ab.py [--matrix stencil|irregular] [--thin 16,128] [--rounds 3]

A cop20k_A stand-in (stencil) or cop20k_irregular_surrogate with repeated
columns removed, a diagonal entry added where one is missing and the diagonal
made dominant (so the factors stay finite).  Forms, timed with bench.py's
discipline as scripts/trsm_ab.py does (copies of (matrix, plans, F) rotated;
the launches of `steps` factorisations captured into one hipGraph on a side
stream; a replay timed with device events after untimed stabilising replays),
the forms alternating within each round:

  auto      chain="auto": thin runs in the one-block kernel, wide levels as grids
  off       chain="off":  one launch per level
  all       chain="all":  every level in the one-block kernel, one launch
  thinN     chain="auto" with the thin-level threshold at N rows
  trsm      the lower solve of the same pattern at K = 32, for scale
  spmm      A X of the same pattern at K = 32, for scale

Before anything is timed every form is compared bit for bit with `auto`, and
`auto` with the numpy loop on the first --check-rows rows.  Prints one JSON
line.
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


def loop_rows(rp, ci, va, nrows):
    """The loop of include/smfv.h on rows [0, nrows): f of those rows, in CSR order."""
    import numpy as np
    f = np.array(va[:rp[nrows]])
    diag = {}
    with np.errstate(all="ignore"):
        for i in range(nrows):
            s, e = int(rp[i]), int(rp[i + 1])
            cols = ci[s:e].tolist()
            pos = {c: t for t, c in enumerate(cols)}
            diag[i] = s + pos[i]
            w = f[s:e]
            for k, t in sorted((c, t) for t, c in enumerate(cols) if c < i):
                w[t] = w[t] / f[diag[k]]
                for q in range(int(rp[k]), int(rp[k + 1])):
                    r = pos.get(int(ci[q])) if ci[q] > k else None
                    if r is not None:
                        prod = w[t] * f[q]
                        w[r] = w[r] - prod
    return f


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("stencil", "irregular"), default="stencil")
    ap.add_argument("--thin", default="16,128", help="thresholds tried beside the default (rows)")
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
        raise SystemExit("ilu0_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K = 32
    A = inputs.cop20k_surrogate() if args.matrix == "stencil" else inputs.cop20k_irregular_surrogate()
    m = A.numRows
    rp0, ci0 = np.asarray(A.rowPtr, np.int64), np.asarray(A.colIndices, np.int64)
    r0 = np.repeat(np.arange(m), np.diff(rp0))
    # repeated columns removed (the first value stays), a diagonal entry where one is missing
    key = np.concatenate([r0 * m + ci0, np.arange(m) * (m + 1)])
    val = np.concatenate([np.asarray(A.values, np.float64), np.zeros(m)])
    key, first = np.unique(key, return_index=True)
    r, ci, va = key // m, key % m, val[first]
    nnz = int(key.size)
    repeats = int(ci0.size - np.unique(r0 * m + ci0).size)
    added = nnz - (int(ci0.size) - repeats)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=m))
    off = ci != r
    va[~off] = 1.0 + np.bincount(r[off], np.abs(va[off]), minlength=m)
    A = inputs.SparseMatrix(values=va, colIndices=ci.astype(np.int32), rowPtr=rp.astype(np.int32), numRows=m, numCols=m)
    X = inputs.generateLargeFatVector(m, K)

    forms = {"auto": {}, "off": {"chain": "off"}, "all": {"chain": "all"}}
    for t in (int(v) for v in args.thin.split(",") if v):
        forms[f"thin{t}"] = {"thin_rows": t}
    host = smfv.ilu0_analyse(A)
    plan_bytes = 8 * host["steps"] + 4 * (host["steps"] + 1) + 8 * host["pairs"] + 12 * m
    ncopies = max(1, min(12, math.ceil(args.cold_bytes / (plan_bytes + 16 * nnz)) + 1))

    copies = []
    for _ in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        c = {f: smfv.Ilu0Plan(dA, **kw) for f, kw in forms.items()}
        c["trsm"] = smfv.TrsmPlan(dA, K, "lower")
        c["spmm"] = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K)
        c["F"] = torch.empty_like(dA.values)
        c["X"] = torch.from_numpy(X).to(dev)
        c["Y"] = torch.empty((m, K), dtype=torch.float64, device=dev)
        copies.append(c)
    c0 = copies[0]
    stats = {f: c0[f].stats() for f in forms}

    # every form against auto, auto against the loop on the first rows
    ref = c0["auto"].factor().clone()
    torch.cuda.synchronize()
    agree = {}
    for f in forms:
        F = c0[f].factor(c0["F"])
        torch.cuda.synchronize()
        agree[f] = bool(torch.equal(F.view(torch.int64), ref.view(torch.int64)))
    n_chk = min(args.check_rows, m)
    fh = loop_rows(rp, ci, va, n_chk)
    refh = ref.cpu().numpy()
    check = bool(np.array_equal(refh[:rp[n_chk]].view(np.uint64), fh.view(np.uint64))) and bool(np.isfinite(refh).all())

    def step(form: str, i: int) -> None:
        c = copies[i % ncopies]
        if form == "spmm":
            c["spmm"].run(c["X"], c["Y"])
        elif form == "trsm":
            c["trsm"].solve(c["X"], c["Y"])
        else:
            c[form].factor(c["F"])

    names = list(forms) + ["trsm", "spmm"]
    launches = {f: stats[f]["launches"] for f in forms}
    launches["trsm"] = c0["trsm"].stats()["launches"]
    steps = {f: max(2, min(args.max_steps, args.nodes // max(1, launches[f]))) for f in launches}
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
        return e0.elapsed_time(e1) * 1e3 / steps[form]  # us per factorisation / solve / product

    us = {form: [] for form in names}
    for _ in range(args.rounds):
        for form in names:
            us[form].append(round(timed(form), 2))
    med = {form: statistics.median(v) for form, v in us.items()}
    keys = ("levels", "widest_level", "launches", "chain_launches", "chain_rows", "chain_max_levels", "thin_rows",
            "steps", "pairs", "max_steps_per_row", "max_pairs_per_row", "long_rows", "plan_bytes", "analysis_ms")
    levels = stats["auto"]["levels"]
    print(json.dumps({
        "what": f"ILU(0) of the cop20k {args.matrix} stand-in, us per factorisation (copies rotated); trsm / spmm at K = 32",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "copies_rotated": ncopies, "m": m, "nnz": nnz,
        "repeated_entries_removed": repeats, "diagonal_entries_added": added, "steps_per_graph": steps, "us": us, "median_us": med,
        "us_per_level": {f: round(med[f] / max(1, levels), 3) for f in list(forms) + ["trsm"]},
        "plan_stats": {f: {k: stats[f][k] for k in keys} for f in forms}, "host_analysis": host,
        "forms_bitwise_equal_auto": agree, "auto_bitwise_vs_loop_rows": n_chk, "auto_bitwise_vs_loop": check}))
    if not (check and all(agree.values())):
        raise SystemExit("ilu0_ab: the forms disagree, or auto differs from the loop")


if __name__ == "__main__":
    main()
