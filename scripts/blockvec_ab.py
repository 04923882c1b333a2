#!/usr/bin/env python3
"""A/B of the block-vector kernels (smfv_coldot_f64, smfv_col_axpy_f64,
smfv_col_xpay_f64, smfv_pcg_update_f64) against their torch expressions and a
copy, and of one BlockPCG iteration against the torch loop of
scripts/reorder_ab.py.

    python scripts/blockvec_ab.py [--rounds 3] [--no-pcg]

m = 121,192 (the cop20k stencil stand-in, prepared as scripts/reorder_ab.py
does), K = 32.  Protocol of scripts/reorder_ab.py: sets of blocks rotated so
that a call's operands come from beyond the Infinity Cache; the launches of
`steps` calls captured into one hipGraph on a side stream; a replay timed with
device events after 0.1 s of untimed replays; the forms alternating within
each of the rounds.

  coldot            smfv_coldot_f64 (two launches)
  torch_dot         (X * Y).sum(0)
  stream_copy       smfv_stream_copy of one block: as many bytes moved as coldot reads
  axpy / torch_axpy           Y += s X      against  Y += (num / den) * X
  xpay / torch_xpay           Y = X + s Y   against  P = Z + (num / den) * P
  pcg_update / three_calls    the fused pass against axpy, axpy, coldot

One PCG iteration (unless --no-pcg; nothing rotated: the same blocks every
iteration, as in a solve), for the natural and the multicolour ILU(0):
BlockPCG.iterate launched eagerly, the same captured in a graph, and the torch
loop of scripts/reorder_ab.py launched eagerly, in the same run.

Before anything is timed: coldot equals smfv_coldot_host on the same data,
the fused update equals the three calls, a captured BlockPCG equals the eager
one, all bit for bit; and BlockPCG reaches the tolerance in the iterations of
the torch loop, give or take one.  SMFV_LIB=<another build> times that build
(the non-temporal-load build of profiles/blockvec/README.md).  Prints one JSON
line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STABILIZE_S = 0.1
TOL = 1e-8


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=6, help="sets of four blocks rotated (31 MB a block)")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--pcg-iters", type=int, default=20)
    ap.add_argument("--no-pcg", action="store_true")
    args = ap.parse_args()

    import ctypes

    import numpy as np
    import torch

    import sparsematrixmultiplicationmpi_amd as smfv
    from reorder_ab import prepared
    from sparsematrixmultiplicationmpi_amd._lib import call, lib
    from sparsematrixmultiplicationmpi_amd.engine import coldot_workspace_doubles, stream_handle

    if not torch.cuda.is_available():
        raise SystemExit("blockvec_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K = 32
    A = prepared("stencil")
    m = A.numRows
    rng = np.random.default_rng(5)
    nbytes = m * K * 8
    i64 = lambda T: T.contiguous().view(torch.int64)  # noqa: E731
    same = lambda a, b: bool(torch.equal(i64(a), i64(b)))  # noqa: E731

    ns = args.sets
    host = [rng.uniform(-1, 1, (m, K)) for _ in range(4)]
    sets = [[torch.from_numpy(h).to(dev) for h in host] for _ in range(ns)]  # P, Q, X, R of every set
    num = torch.from_numpy(rng.uniform(0.5, 2, K)).to(dev)
    den = torch.from_numpy(rng.uniform(0.5, 2, K)).to(dev)
    out = torch.empty(K, dtype=torch.float64, device=dev)
    ws = torch.empty(coldot_workspace_doubles(m, K), dtype=torch.float64, device=dev)

    # ---- bit-exactness, before anything is timed
    P, Q, Xb, Rb = sets[0]
    want = np.empty(K)
    assert lib.smfv_coldot_host(m, K, host[0].ctypes.data, K, host[1].ctypes.data, K, want.ctypes.data) == 0
    checks = {"coldot_equals_host_rule": same(smfv.coldot(P, Q, out, workspace=ws), torch.from_numpy(want).to(dev))}
    x1, r1, x2, r2 = Xb.clone(), Rb.clone(), Xb.clone(), Rb.clone()
    rr1 = smfv.pcg_update(num, den, P, Q, x1, r1, workspace=ws).clone()
    smfv.col_axpy(num, den, P, x2)
    smfv.col_axpy(num, den, Q, r2, negate=True)
    checks["fused_equals_three_calls"] = same(rr1, smfv.coldot(r2, r2)) and same(x1, x2) and same(r1, r2)
    checks["torch_dot_differs_in_bits"] = not same((P * Q).sum(0), out)
    del x1, r1, x2, r2
    torch.cuda.synchronize()

    def captured(fn, nsteps, warm):
        for i in range(warm):
            fn(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(nsteps):
                    fn(i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        return g

    def timed(g, nsteps) -> float:
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
        return e0.elapsed_time(e1) * 1e3 / nsteps  # us per call

    S = lambda i: sets[i % ns]  # noqa: E731

    fresh = [None] * ns  # the results of torch's P = Z + beta * P: new tensors, as the torch loop makes them

    def torch_xpay(i):
        # never rebind an entry of `sets`: the graphs captured before hold its address, and torch
        # empties its allocator cache when the next capture begins
        fresh[i % ns] = S(i)[1] + (num / den) * S(i)[0]

    def three_calls(i):
        p, q, x, r = S(i)
        smfv.col_axpy(num, den, p, x)
        smfv.col_axpy(num, den, q, r, negate=True)
        smfv.coldot(r, r, out, workspace=ws)

    def torch_axpy(i):
        y = S(i)[2]
        y += (num / den) * S(i)[0]

    forms = {
        "coldot": lambda i: smfv.coldot(S(i)[0], S(i)[1], out, workspace=ws),
        "torch_dot": lambda i: (S(i)[0] * S(i)[1]).sum(0),
        "stream_copy": lambda i: call("smfv_stream_copy", S(i)[2].data_ptr(), S(i)[0].data_ptr(), nbytes, stream_handle(None)),
        "axpy": lambda i: smfv.col_axpy(num, den, S(i)[0], S(i)[2]),
        "torch_axpy": torch_axpy,
        "xpay": lambda i: smfv.col_xpay(num, den, S(i)[1], S(i)[0]),
        "torch_xpay": torch_xpay,
        "pcg_update": lambda i: smfv.pcg_update(num, den, *S(i), rr=out, workspace=ws),
        "three_calls": three_calls,
    }
    # bytes a call moves by its algorithm (read + written)
    moved = {"coldot": 2, "torch_dot": 2, "stream_copy": 2, "axpy": 3, "torch_axpy": 3, "xpay": 3, "torch_xpay": 3,
             "pcg_update": 6, "three_calls": 8}
    graphs = {f: captured(fn, args.steps, ns) for f, fn in forms.items()}
    us = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            us[f].append(round(timed(graphs[f], args.steps), 2))
    med = {f: statistics.median(v) for f, v in us.items()}
    res = {
        "what": f"block-vector kernels, m = {m}, K = {K}, us per call ({ns} sets of blocks rotated, {args.steps} calls per graph)",
        "device": torch.cuda.get_device_name(0), "library": os.environ.get("SMFV_LIB") or "libsmfv.so", "rounds": args.rounds,
        "block_bytes": nbytes, "coldot_rule": smfv.coldot_rule(), "checks": checks, "us": us, "median_us": med,
        "spread_over_median": {f: round((max(v) - min(v)) / med[f], 4) for f, v in us.items()},
        "TBps_algorithmic": {f: round(moved[f] * nbytes / med[f] / 1e6, 3) for f in med},
        "ratio": {"coldot_over_torch_dot": round(med["coldot"] / med["torch_dot"], 3),
                  "coldot_over_stream_copy": round(med["coldot"] / med["stream_copy"], 3),
                  "axpy_over_torch": round(med["axpy"] / med["torch_axpy"], 3),
                  "xpay_over_torch": round(med["xpay"] / med["torch_xpay"], 3),
                  "fused_over_three_calls": round(med["pcg_update"] / med["three_calls"], 3)},
    }
    del graphs, sets
    torch.cuda.empty_cache()
    if not all(checks.values()):
        print(json.dumps(res))
        raise SystemExit("blockvec_ab: a bit-exactness check failed")

    # ---- one PCG iteration: BlockPCG eager and captured against the torch loop
    if not args.no_pcg:
        dA = smfv.DeviceCSR(A, dev)
        spmm = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K)
        Bm = torch.from_numpy(rng.uniform(-1, 1, (m, K))).to(dev)
        bnorm = Bm.norm(dim=0)
        Qt, Zt = torch.empty_like(Bm), torch.empty_like(Bm)

        def torch_pcg(M, iters=None, max_iters=500):
            """The loop of scripts/reorder_ab.py.  iters None: until every column's relative residual is
            <= TOL (a host read-back every iteration); else `iters` iterations, no read-back, timed."""
            Xk, Rk = torch.zeros_like(Bm), Bm.clone()
            M.apply(Rk, Zt)
            Pk = Zt.clone()
            rz = (Rk * Zt).sum(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            it = 0
            while it < (iters if iters is not None else max_iters):
                spmm.run(Pk, Qt)
                alpha = rz / (Pk * Qt).sum(0)
                Xk += alpha * Pk
                Rk -= alpha * Qt
                it += 1
                if iters is None and float((Rk.norm(dim=0) / bnorm).max()) <= TOL:
                    break
                M.apply(Rk, Zt)
                rz_new = (Rk * Zt).sum(0)
                Pk = Zt + (rz_new / rz) * Pk
                rz = rz_new
            e1.record()
            torch.cuda.synchronize()
            return it, e0.elapsed_time(e1) * 1e3 / max(1, it)

        def true_rel(Xk):
            spmm.run(Xk, Qt)
            return float(((Bm - Qt).norm(dim=0) / bnorm).max())

        pcg = {}
        n = args.pcg_iters
        for w in ("nat", "mc"):
            M = smfv.Ilu0Preconditioner(dA, K, reorder=None if w == "nat" else "multicolor")
            solver = smfv.BlockPCG(spmm, K, M)
            Xs, its, rel = solver.solve(Bm, tol=TOL, max_iters=500)
            Xe = Xs.clone()
            Xg, itg, _ = solver.solve(Bm, tol=TOL, max_iters=500, graph=True)
            it_torch, _ = torch_pcg(M)
            ok = {"captured_equals_eager": itg == its and same(Xg, Xe), "iterations_as_torch_loop": abs(its - it_torch) <= 1}
            g = torch.cuda.CUDAGraph()
            solver.start(Bm)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    solver.iterate(n, side)  # n is even: the rz buffers end where they began
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            t = {"blockpcg_eager": [], "blockpcg_graph": [], "torch_loop": []}
            for _ in range(args.rounds):
                solver.start(Bm)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                solver.iterate(n)
                e1.record()
                torch.cuda.synchronize()
                t["blockpcg_eager"].append(round(e0.elapsed_time(e1) * 1e3 / n, 1))
                solver.start(Bm)
                t["blockpcg_graph"].append(round(timed(g, n), 1))
                t["torch_loop"].append(round(torch_pcg(M, n)[1], 1))
            md = {k: statistics.median(v) for k, v in t.items()}
            pcg[w] = {"iterations": its, "iterations_torch_loop": it_torch, "true_relative_residual": true_rel(Xe),
                      "worst_rr_over_bb": float(rel.max()), "checks": ok, "us_per_iteration": t, "median_us_per_iteration": md,
                      "graph_over_torch_loop": round(md["blockpcg_graph"] / md["torch_loop"], 3),
                      "eager_over_torch_loop": round(md["blockpcg_eager"] / md["torch_loop"], 3)}
            del g, solver, M
        res["pcg"] = {"what": f"one PCG iteration, K = {K} right-hand sides, {n} iterations timed per form, the same blocks every "
                              "iteration; A P (SpmmPlan), Ilu0Preconditioner.apply, two dots and two updates", **pcg}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
