#!/usr/bin/env python3
"""A/B of Y = A^T X through a transposed plan (SMFV_PLAN_TRANSPOSE) against
what a caller does without it: a second, explicitly transposed CSR.

    python scripts/transpose_ab.py [--matrix stencil|irregular] [--steps 200] [--warmup 20] [--rounds 3]

cop20k_A stand-in (stencil) or cop20k_irregular_surrogate, K = 32, ROWWISE.
Forms, timed with bench.py's discipline (rotate over enough copies of (plans,
X, Y) that every launch streams from HBM; `steps` launches captured into one
hipGraph on a side stream; a replay timed with device events after untimed
stabilising replays), the forms alternating within each round:

  a        fwd.run(X, Y)              forward product of A
  b        tr.run(X, Y)               transposed plan of A (Y = A^T X)
  c        exp.run(X, Y)              forward product of an explicitly
                                      transposed DeviceCSR (inputs.csr_transpose):
                                      the baseline for (b) -- same pattern, same
                                      kernels
  d_b / d_c           bind + execute per step, snapshot values: (b) pays
                      k_permute_vals (about 20 B per non-zero) before the gather
  d_b_live / d_c_live the same with live_values (for (c) the bind is a no-op)

(b) is checked bit for bit against (c) and against the oracle on a row sample
before anything is timed.  Prints one JSON line.
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
FORMS = ("a", "b", "c", "d_b", "d_c", "d_b_live", "d_c_live")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("stencil", "irregular"), default="stencil")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cold-bytes", type=float, default=1.0e9)
    ap.add_argument("--sample-rows", type=int, default=512)
    args = ap.parse_args()

    import numpy as np
    import torch

    import sparsematrixmultiplicationmpi_amd as smfv
    from oracle import oracle
    from sparsematrixmultiplicationmpi_amd import inputs

    if not torch.cuda.is_available():
        raise SystemExit("transpose_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K, V = 32, smfv.Variant.ROWWISE
    A = inputs.cop20k_surrogate() if args.matrix == "stencil" else inputs.cop20k_irregular_surrogate()
    At, _ = inputs.csr_transpose(A)
    m, n, nnz = A.numRows, A.numCols, A.nnz
    X = inputs.generateLargeFatVector(max(m, n), K)
    spmm_b = 12 * nnz + 4 * (m + 1) + 8 * n * K + 8 * m * K
    model = {"product": spmm_b, "permute_pass": 20 * nnz, "snapshot_gather_at_least": 16 * nnz}
    ncopies = max(1, min(16, math.ceil(args.cold_bytes / spmm_b) + 1))

    copies = []
    for _ in range(ncopies):
        dA, dAt = smfv.DeviceCSR(A, dev), smfv.DeviceCSR(At, dev)
        copies.append({"fwd": smfv.SpmmPlan(V, dA, K), "tr": smfv.SpmmPlan(V, dA, K, transpose=True),
                       "exp": smfv.SpmmPlan(V, dAt, K),
                       "tr_live": smfv.SpmmPlan(V, dA, K, transpose=True, live_values=True),
                       "exp_live": smfv.SpmmPlan(V, dAt, K, live_values=True),
                       "Xn": torch.from_numpy(X[:n]).to(dev), "Xm": torch.from_numpy(X[:m]).to(dev),
                       "Ym": torch.empty((m, K), dtype=torch.float64, device=dev),
                       "Yn": torch.empty((n, K), dtype=torch.float64, device=dev)})
    c0 = copies[0]
    keys = ("tiled", "kernel", "tiles", "staged_rows", "direct_rows", "ws_geom", "paired_rows", "snapshot_entries",
            "live_values", "bind_descriptors", "plan_bytes", "analysis_ms")
    stats = {k: {q: c0[k].stats()[q] for q in keys} for k in ("fwd", "tr", "exp", "tr_live", "exp_live")}
    same_plan = all(stats["tr"][q] == stats["exp"][q] for q in keys if q not in ("plan_bytes", "analysis_ms"))

    # (b) against (c), whole result, and against the oracle on a row sample of A^T
    c0["tr"].run(c0["Xm"], c0["Yn"])
    Yc = torch.empty_like(c0["Yn"])
    c0["exp"].run(c0["Xm"], Yc)
    torch.cuda.synchronize()
    b_equals_c = bool(torch.equal(c0["Yn"].view(torch.int64), Yc.view(torch.int64)))
    rows = np.unique(np.random.default_rng(11).integers(0, n, args.sample_rows))
    rp = At.rowPtr.astype(np.int64)
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows])
    rps = np.zeros(rows.size + 1, np.int32)
    rps[1:] = np.cumsum(rp[rows + 1] - rp[rows])
    want = oracle.spmm("sequential", rps, At.colIndices[idx], At.values[idx], X[:m])
    got = c0["Yn"][torch.from_numpy(rows).to(dev)].cpu().numpy()
    check = bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))

    def step(form: str, i: int) -> None:
        c = copies[i % ncopies]
        if form == "a":
            c["fwd"].run(c["Xn"], c["Ym"])
        elif form == "b":
            c["tr"].run(c["Xm"], c["Yn"])
        elif form == "c":
            c["exp"].run(c["Xm"], c["Yn"])
        else:
            p = c[{"d_b": "tr", "d_c": "exp", "d_b_live": "tr_live", "d_c_live": "exp_live"}[form]]
            p.bind_values(torch.cuda.current_stream())
            p.run(c["Xm"], c["Yn"])

    graphs = {}
    for form in FORMS:
        for i in range(max(args.warmup, ncopies)):
            step(form, i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(args.steps):
                    step(form, i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[form] = g

    def timed(g) -> float:
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
        return e0.elapsed_time(e1) * 1e3 / args.steps  # us per step

    us = {form: [] for form in FORMS}
    for _ in range(args.rounds):
        for form in FORMS:
            us[form].append(round(timed(graphs[form]), 3))
    med = {form: statistics.median(v) for form, v in us.items()}
    # leave every plan bound eagerly (the captured binds ran at replay)
    for c in copies:
        for k in ("tr", "exp", "tr_live", "exp_live"):
            c[k].bind_values()
    torch.cuda.synchronize()
    print(json.dumps({
        "what": f"Y = A^T X, cop20k {args.matrix} stand-in, K = 32, ROWWISE, us per step (cold: copies rotated)",
        "device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds,
        "copies_rotated": ncopies, "m": m, "n": n, "nnz": nnz,
        "forms": {"a": "forward run of A", "b": "transposed run of A", "c": "forward run of an explicit A^T",
                  "d_b": "bind + run, transposed plan", "d_c": "bind + run, explicit A^T",
                  "d_b_live": "bind + run, transposed plan, live_values",
                  "d_c_live": "bind + run, explicit A^T, live_values (bind is a no-op)"},
        "us": us, "median_us": med,
        "b_over_c": round(med["b"] / med["c"], 4), "b_over_a": round(med["b"] / med["a"], 4),
        # a bind's time: the bind + run step less the run alone; with live
        # values (c)'s bind is a no-op, so d_b_live - d_c_live is k_permute_vals
        "bind_us": {"b": round(med["d_b"] - med["b"], 3), "c": round(med["d_c"] - med["c"], 3),
                    "b_live_minus_c_live": round(med["d_b_live"] - med["d_c_live"], 3)},
        "model_bytes": model, "plan_stats": stats, "b_and_c_same_plan": same_plan,
        "b_bitwise_equals_c": b_equals_c, "b_check_rows": int(rows.size), "b_bitwise_vs_oracle": check}))
    if not (check and b_equals_c):
        raise SystemExit("transpose_ab: the transposed result differs from the explicit transpose / the oracle")


if __name__ == "__main__":
    main()
