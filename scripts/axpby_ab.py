#!/usr/bin/env python3
"""A/B of Y = alpha*A*X + beta*Y on the cop20k_A stand-in, K = 32, ROWWISE,
beta != 0: what the fused epilogue buys over the forms a caller has without it.

    python scripts/axpby_ab.py [--steps 200] [--warmup 20] [--rounds 3]

Four forms, timed with bench.py's discipline (rotate over enough copies of
(plan, X, Y) that every launch streams from HBM; `steps` launches captured
into one hipGraph on a side stream; a replay timed with device events after
untimed stabilising replays), the forms alternating within each round:

  a  plan.run(X, Y)                       the plain product (94 MB per step)
  b  fused.run_axpby(X, Y, alpha, beta)   the epilogue in the kernel's store (125 MB)
  c  two_pass.run_axpby(...)              axpby="two_pass": scratch + k_axpby (187 MB)
  d  plan.run(X, S); Y.mul_(beta).add_(S, alpha=alpha)
                                          what a caller can do without the
                                          feature (> 187 MB: two framework passes)

(b) is checked against the oracle on a row sample before anything is timed.
Prints one JSON line: per form the per-step microseconds of every round and
their median, the ratios b/c and b/d, and the byte model.
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

ALPHA, BETA = 1.0 / 3.0, -0.7
STABILIZE_S = 0.1


def main() -> None:
    ap = argparse.ArgumentParser()
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
        raise SystemExit("axpby_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K, V = 32, smfv.Variant.ROWWISE
    A = inputs.cop20k_surrogate()
    m, n, nnz = A.numRows, A.numCols, A.nnz
    X = inputs.generateLargeFatVector(n, K)
    Y0 = np.random.default_rng(7).uniform(-1, 1, (m, K))
    # bytes per step: CSR + X in, Y out (+ Y in, + the scratch both ways)
    spmm_b = 12 * nnz + 4 * (m + 1) + 8 * n * K + 8 * m * K
    y_b = 8 * m * K
    model = {"plain": spmm_b, "fused": spmm_b + y_b, "two_pass_or_unfused_best": spmm_b + 3 * y_b}
    ncopies = max(1, min(16, math.ceil(args.cold_bytes / spmm_b) + 1))

    copies = []
    for _ in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        copies.append({"plain": smfv.SpmmPlan(V, dA, K), "fused": smfv.SpmmPlan(V, dA, K, axpby=True),
                       "two_pass": smfv.SpmmPlan(V, dA, K, axpby="two_pass"),
                       "X": torch.from_numpy(X).to(dev), "Y": torch.from_numpy(Y0).to(dev),
                       "S": torch.empty((m, K), dtype=torch.float64, device=dev)})
    c0 = copies[0]
    modes = {k: c0[k].epilogue_mode for k in ("plain", "fused", "two_pass")}
    assert modes == {"plain": None, "fused": "fused", "two_pass": "two_pass"}, modes
    stats = c0["fused"].stats()

    # (b) against the oracle on a row sample, from a fresh Y0
    rows = np.unique(np.random.default_rng(11).integers(0, m, args.sample_rows))
    rp = A.rowPtr.astype(np.int64)
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows])
    rps = np.zeros(rows.size + 1, np.int32)
    rps[1:] = np.cumsum(rp[rows + 1] - rp[rows])
    S = oracle.spmm("sequential", rps, A.colIndices[idx], A.values[idx], X)
    want = ALPHA * S + BETA * Y0[rows]
    c0["fused"].run_axpby(c0["X"], c0["Y"], ALPHA, BETA)
    torch.cuda.synchronize()
    got = c0["Y"][torch.from_numpy(rows).to(dev)].cpu().numpy()
    check = bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))
    c0["Y"].copy_(torch.from_numpy(Y0))

    def step(form: str, i: int) -> None:
        c = copies[i % ncopies]
        if form == "a":
            c["plain"].run(c["X"], c["Y"])
        elif form == "b":
            c["fused"].run_axpby(c["X"], c["Y"], ALPHA, BETA)
        elif form == "c":
            c["two_pass"].run_axpby(c["X"], c["Y"], ALPHA, BETA)
        else:
            c["plain"].run(c["X"], c["S"])
            c["Y"].mul_(BETA).add_(c["S"], alpha=ALPHA)

    graphs = {}
    for form in "abcd":
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

    us = {form: [] for form in "abcd"}
    for _ in range(args.rounds):
        for form in "abcd":
            us[form].append(round(timed(graphs[form]), 3))
    med = {form: statistics.median(v) for form, v in us.items()}
    print(json.dumps({
        "what": "Y = alpha*A*X + beta*Y, cop20k_A surrogate, K = 32, ROWWISE, us per step (cold: copies rotated)",
        "device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds,
        "copies_rotated": ncopies, "alpha": ALPHA, "beta": BETA,
        "forms": {"a": "run()", "b": "fused run_axpby", "c": "two-pass run_axpby",
                  "d": "run() into scratch + Y.mul_(beta).add_(S, alpha=alpha)"},
        "us": us, "median_us": med,
        "b_over_c": round(med["b"] / med["c"], 4), "b_over_d": round(med["b"] / med["d"], 4),
        "b_over_a": round(med["b"] / med["a"], 4),
        "model_bytes": model, "fused_kernel": stats["kernel"], "fused_tiles": stats["tiles"],
        "fused_check_rows": int(rows.size), "fused_bitwise_vs_oracle": check}))
    if not check:
        raise SystemExit("axpby_ab: the fused result differs from the oracle on the row sample")


if __name__ == "__main__":
    main()
