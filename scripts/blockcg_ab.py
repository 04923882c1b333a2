#!/usr/bin/env python3
"""A/B of the coupled-block kernels (smfv_gram_f64, smfv_block_mul_f64,
smfv_small_solve_f64) against their torch expressions and a copy, and of
CoupledBlockPCG against BlockPCG.

    python scripts/blockcg_ab.py [--rounds 3] [--no-pcg] [--ks 32,128]

m = 121,192 (the cop20k stencil stand-in, prepared as scripts/reorder_ab.py
does), K = 32 and K = 128.  Protocol of scripts/blockvec_ab.py: sets of blocks
rotated so that a call's operands come from beyond the Infinity Cache; the
launches of `steps` calls captured into one hipGraph on a side stream; a replay
timed with device events after 0.1 s of untimed replays; the forms alternating
within each of the rounds.

  gram / torch_gram           smfv_gram_f64 (two launches)  against  X.T @ Y
  block_mul / torch_addmm     Y = Z + X C                   against  torch.addmm(Z, X, C)
  stream_copy                 smfv_stream_copy of one block (it moves two blocks' bytes)
  small_solve                 smfv_small_solve_f64 of a K x K system with K right-hand sides

Then (unless --no-pcg), K = 32 under the multicolour ILU(0), on two matrices --
the stand-in, and the same pattern with its diagonal scaled down until BlockPCG
needs at least 50 iterations (or stops converging) --: the iterations and the time of a whole
solve to 1e-8 (captured iterations, one residual read per iteration), and the
time of one captured iteration, for BlockPCG and CoupledBlockPCG in the same
run.

Before anything is timed: gram equals smfv_gram_host and small_solve equals
smfv_small_solve_host on the same data, block_mul equals the numpy rule on the
first and last rows, a captured CoupledBlockPCG solve equals the eager one, all
bit for bit.  Prints one JSON line per K and one for the solvers.
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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--ks", default="32,128")
    ap.add_argument("--pcg-iters", type=int, default=10)
    ap.add_argument("--no-pcg", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import sparsematrixmultiplicationmpi_amd as smfv
    from reorder_ab import prepared
    from sparsematrixmultiplicationmpi_amd import inputs
    from sparsematrixmultiplicationmpi_amd._lib import call, lib
    from sparsematrixmultiplicationmpi_amd.engine import stream_handle

    if not torch.cuda.is_available():
        raise SystemExit("blockcg_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    A = prepared("stencil")
    m = A.numRows
    rng = np.random.default_rng(5)
    i64 = lambda T: T.contiguous().view(torch.int64)  # noqa: E731
    same = lambda a, b: bool(torch.equal(i64(a), i64(b)))  # noqa: E731

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

    for K in [int(k) for k in args.ks.split(",")]:
        nbytes = m * K * 8
        ns = max(3, -(-1_000_000_000 // (3 * nbytes)))  # sets of three blocks: a gigabyte rotated
        host = [rng.uniform(-1, 1, (m, K)) for _ in range(3)]
        sets = [[torch.from_numpy(h).to(dev) for h in host] for _ in range(ns)]  # X, Y / Z, the output
        Ch = rng.uniform(-1, 1, (K, K)) + K * np.eye(K)
        C = torch.from_numpy(Ch).to(dev)
        Hh = rng.uniform(-1, 1, (K, K))
        H = torch.from_numpy(Hh).to(dev)
        G, Cs = torch.empty((K, K), dtype=torch.float64, device=dev), torch.empty((K, K), dtype=torch.float64, device=dev)
        ws = torch.empty(smfv.gram_workspace_doubles(m, K, K), dtype=torch.float64, device=dev)

        # ---- bit-exactness, before anything is timed
        X, Y, Z = sets[0]
        want = np.empty((K, K))
        assert lib.smfv_gram_host(m, K, K, host[0].ctypes.data, K, host[1].ctypes.data, K, want.ctypes.data, K) == 0
        checks = {"gram_equals_host_rule": same(smfv.gram(X, Y, G, workspace=ws), torch.from_numpy(want).to(dev))}
        checks["torch_gram_differs_in_bits"] = not same(X.T @ Y, G)
        assert lib.smfv_small_solve_host(K, K, Ch.ctypes.data, K, Hh.ctypes.data, K, want.ctypes.data, K) == 0
        checks["small_solve_equals_host_rule"] = same(smfv.small_solve(C, H, Cs), torch.from_numpy(want).to(dev))
        rows = np.r_[0:3000, m - 3000:m]
        acc = host[1][rows].copy()
        for l in range(K):
            acc = acc + host[0][rows, l:l + 1] * Ch[l][None, :]
        got = smfv.block_mul(X, C, Y)
        checks["block_mul_equals_numpy_rule"] = same(got[torch.from_numpy(rows).to(dev)], torch.from_numpy(acc).to(dev))
        del got
        torch.cuda.synchronize()

        S = lambda i: sets[i % ns]  # noqa: E731
        fresh = [None] * ns  # torch's results are new tensors; never rebind an entry of `sets` (captured addresses)

        def torch_gram(i):
            fresh[i % ns] = S(i)[0].T @ S(i)[1]

        def torch_addmm(i):
            fresh[i % ns] = torch.addmm(S(i)[1], S(i)[0], C)

        forms = {
            "gram": lambda i: smfv.gram(S(i)[0], S(i)[1], G, workspace=ws),
            "torch_gram": torch_gram,
            "block_mul": lambda i: smfv.block_mul(S(i)[0], C, S(i)[1], S(i)[2]),
            "torch_addmm": torch_addmm,
            "stream_copy": lambda i: call("smfv_stream_copy", S(i)[2].data_ptr(), S(i)[0].data_ptr(), nbytes, stream_handle(None)),
            "small_solve": lambda i: smfv.small_solve(C, H, Cs),
        }
        moved = {"gram": 2, "torch_gram": 2, "block_mul": 3, "torch_addmm": 3, "stream_copy": 2}  # blocks read + written
        graphs = {f: captured(fn, args.steps, ns) for f, fn in forms.items()}
        us = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f in forms:
                us[f].append(round(timed(graphs[f], args.steps), 2))
        med = {f: statistics.median(v) for f, v in us.items()}
        res = {
            "what": f"coupled-block kernels, m = {m}, K = {K}, us per call ({ns} sets of blocks rotated, {args.steps} calls per graph)",
            "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block_bytes": nbytes, "checks": checks, "us": us,
            "median_us": med, "spread_over_median": {f: round((max(v) - min(v)) / med[f], 4) for f, v in us.items()},
            "MB_moved": {f: round(moved[f] * nbytes / 1e6, 1) for f in moved},
            "TBps_algorithmic": {f: round(moved[f] * nbytes / med[f] / 1e6, 3) for f in moved},
            "Gflops": {f: round(2.0 * m * K * K / med[f] / 1e3, 1) for f in ("gram", "torch_gram", "block_mul", "torch_addmm")},
            "ratio": {"gram_over_torch": round(med["gram"] / med["torch_gram"], 3),
                      "gram_over_stream_copy": round(med["gram"] / med["stream_copy"], 3),
                      "block_mul_over_torch": round(med["block_mul"] / med["torch_addmm"], 3),
                      "block_mul_over_copy_of_same_bytes": round(med["block_mul"] / (1.5 * med["stream_copy"]), 3)},
        }
        print(json.dumps(res), flush=True)
        del graphs, sets, fresh, forms
        torch.cuda.empty_cache()
        if not all(checks.values()):
            raise SystemExit("blockcg_ab: a bit-exactness check failed")

    # ---- the solvers, K = 32, multicolour ILU(0)
    if args.no_pcg:
        return
    K, n = 32, args.pcg_iters + args.pcg_iters % 2  # an even count: the parity buffers end where they began
    Bm = torch.from_numpy(rng.uniform(-1, 1, (m, K))).to(dev)

    def with_diagonal(f):
        """The stand-in's pattern and off-diagonal values, its diagonal (1 + sum |off-diagonal|) times f."""
        rp, ci = np.asarray(A.rowPtr, np.int64), np.asarray(A.colIndices, np.int64)
        r = np.repeat(np.arange(m), np.diff(rp))
        va = np.asarray(A.values, np.float64).copy()
        va[ci == r] *= f
        return inputs.SparseMatrix(values=va, colIndices=A.colIndices, rowPtr=A.rowPtr, numRows=m, numCols=m)

    def solvers(Ah):
        dA = smfv.DeviceCSR(Ah, dev)
        spmm = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K)
        M = smfv.Ilu0Preconditioner(dA, K, reorder="multicolor")
        return spmm, M, smfv.BlockPCG(spmm, K, M), smfv.CoupledBlockPCG(spmm, K, M)

    out = {}
    f_used, tried = 1.0, []
    for name in ("stand_in", "weak_diagonal"):
        if name == "stand_in":
            spmm, M, col, blk = solvers(A)
        else:
            # the diagonal scaled down until the column-wise solver needs at least 50 iterations; a factor
            # at which it no longer converges in 400 (the matrix is no longer positive definite) ends the search
            spmm, M, col, blk = solvers(A)  # factor 1, kept if no smaller one converges
            for f in (0.9, 0.8, 0.7, 0.6, 0.55, 0.5, 0.45, 0.4, 0.35, 0.3):
                cand = solvers(with_diagonal(f))
                it_f, rel_f = cand[2].solve(Bm, tol=TOL, max_iters=400)[1:]
                tried.append([f, it_f, bool(np.all(rel_f <= TOL * TOL))])
                if not tried[-1][2]:
                    break
                spmm, M, col, blk = cand
                f_used = f
                if it_f >= 50:
                    break
            del cand
        Qt = torch.empty_like(Bm)
        entry = {}
        for form, solver in (("BlockPCG", col), ("CoupledBlockPCG", blk)):
            Xe, its, rel = solver.solve(Bm, tol=TOL, max_iters=1000)
            Xe = Xe.clone()
            Xg, itg, _ = solver.solve(Bm, tol=TOL, max_iters=1000, graph=True)  # captures on the first call
            equal = itg == its and same(Xg, Xe)  # (Xg is the solver's own X: compared before the next start)
            spmm.run(Xe, Qt)
            true_rel = float(((Bm - Qt).norm(dim=0) / Bm.norm(dim=0)).max())
            whole = []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                solver.solve(Bm, tol=TOL, max_iters=1000, graph=True)
                torch.cuda.synchronize()
                whole.append(round((time.perf_counter() - t0) * 1e6, 1))
            g = torch.cuda.CUDAGraph()
            solver.start(Bm)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    solver.iterate(n, side)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            entry[form] = {"iterations": its, "captured_equals_eager": equal,
                           "breakdown": bool(getattr(solver, "breakdown", False)), "true_relative_residual": true_rel,
                           "worst_rr_over_bb": float(np.nanmax(rel)), "solve_us": whole, "graph": g}
            del Xg
        per_it = {f: [] for f in entry}
        for _ in range(args.rounds):
            for form, solver in (("BlockPCG", col), ("CoupledBlockPCG", blk)):
                solver.start(Bm)
                per_it[form].append(round(timed(entry[form]["graph"], n), 1))
        for form in entry:
            del entry[form]["graph"]
            entry[form]["us_per_iteration"] = per_it[form]
            entry[form]["median_us_per_iteration"] = statistics.median(per_it[form])
            entry[form]["median_solve_us"] = statistics.median(entry[form]["solve_us"])
        entry["iterations_ratio"] = round(entry["CoupledBlockPCG"]["iterations"] / entry["BlockPCG"]["iterations"], 3)
        entry["iteration_time_ratio"] = round(entry["CoupledBlockPCG"]["median_us_per_iteration"] /
                                              entry["BlockPCG"]["median_us_per_iteration"], 3)
        entry["solve_time_ratio"] = round(entry["CoupledBlockPCG"]["median_solve_us"] / entry["BlockPCG"]["median_solve_us"], 3)
        if name == "weak_diagonal":
            entry["diagonal_factor"], entry["factors_tried"] = f_used, tried  # [factor, BlockPCG iterations, converged]
        out[name] = entry
        del spmm, M, col, blk
        torch.cuda.empty_cache()
    print(json.dumps({"what": f"BlockPCG against CoupledBlockPCG, m = {m}, K = {K}, multicolour ILU(0), tol {TOL}: whole solves "
                              f"(captured iterations, a residual read every iteration) and one captured iteration ({n} per graph)",
                      "device": torch.cuda.get_device_name(0), "rounds": args.rounds, **out}))


if __name__ == "__main__":
    main()
