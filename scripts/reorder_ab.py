#!/usr/bin/env python3
"""A/B of the natural and the multicolour ordering for the solves, ILU(0) and
the preconditioner apply (smfv_reorder_plan_*, ReorderedCSR,
Ilu0Preconditioner(reorder=...)), and of k_permute_rows against a copy.

    python scripts/reorder_ab.py [--matrix stencil|irregular] [--rounds 3] [--no-pcg] [--no-rows]

A cop20k_A stand-in prepared as scripts/ilu0_ab.py does (repeated columns
removed, a diagonal entry added where one is missing, the diagonal made
dominant), K = 32.  Forms, timed with the protocol of scripts/ilu0_ab.py and
scripts/trsm_ab.py (copies of (matrix, plans, buffers) rotated; the launches
of `steps` executions captured into one hipGraph on a side stream; a replay
timed with device events after 0.1 s of untimed replays), natural and
multicolour forms alternating within each of the rounds:

  nat_lower / mc_lower    the unit lower solve on the factors
  nat_upper / mc_upper    the upper solve
  nat_ilu0 / mc_ilu0      the factorisation
  nat_apply / mc_apply    Ilu0Preconditioner.apply; mc_apply = to_new, both solves, to_old
  mc_apply_nt             mc_apply with non-temporal stores in both permutations
  mc_apply_noperm         both solves in B's numbering, no permutation
  to_new / to_old         k_permute_rows alone (plain stores)
  spmm                    A X of the same pattern, for scale

With the stencil stand-in (unless --no-rows) k_permute_rows at m = 121,192,
K = 32 in both directions with plain and non-temporal stores, against
smfv_stream_copy of the same bytes and torch.index_select into a preallocated
output; and (unless --no-pcg) a plain block PCG in torch on the same matrix
(symmetric, diagonally dominant): iterations to a relative residual of 1e-8
under both orderings and the measured time per iteration.

Before anything is timed: to_old(to_new(X)) == X, non-temporal == plain,
to_new == index_select, and B to_new(X) == to_new(A X), all bit for bit.
Prints one JSON line.
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

STABILIZE_S = 0.1
TOL = 1e-8


def prepared(name):
    """The stand-in as scripts/ilu0_ab.py prepares it."""
    import numpy as np
    from sparsematrixmultiplicationmpi_amd import inputs
    A = inputs.cop20k_surrogate() if name == "stencil" else inputs.cop20k_irregular_surrogate()
    m = A.numRows
    rp0, ci0 = np.asarray(A.rowPtr, np.int64), np.asarray(A.colIndices, np.int64)
    r0 = np.repeat(np.arange(m), np.diff(rp0))
    key = np.concatenate([r0 * m + ci0, np.arange(m) * (m + 1)])
    val = np.concatenate([np.asarray(A.values, np.float64), np.zeros(m)])
    key, first = np.unique(key, return_index=True)
    r, ci, va = key // m, key % m, val[first]
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=m))
    off = ci != r
    va[~off] = 1.0 + np.bincount(r[off], np.abs(va[off]), minlength=m)
    return inputs.SparseMatrix(values=va, colIndices=ci.astype(np.int32), rowPtr=rp.astype(np.int32), numRows=m, numCols=m)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("stencil", "irregular"), default="stencil")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=6000, help="kernel nodes per captured graph, about")
    ap.add_argument("--max-steps", type=int, default=40)
    ap.add_argument("--max-iters", type=int, default=500)
    ap.add_argument("--no-pcg", action="store_true")
    ap.add_argument("--no-rows", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd._lib import call
    from sparsematrixmultiplicationmpi_amd.engine import stream_handle

    if not torch.cuda.is_available():
        raise SystemExit("reorder_ab: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K = 32
    A = prepared(args.matrix)
    m, nnz = A.numRows, A.nnz
    # A's rows are sorted by column (np.unique), and so are A^T's (a stable sort by column)
    t = smfv.csr_transpose(A)[0]
    symmetric = bool(np.array_equal(t.rowPtr, A.rowPtr) and np.array_equal(t.colIndices, A.colIndices)
                     and np.array_equal(t.values, A.values))
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (m, K))

    t0 = time.time()
    copies = []
    for _ in range(args.copies):
        dA = smfv.DeviceCSR(A, dev)
        c = {"A": dA, "nat": smfv.Ilu0Preconditioner(dA, K), "mc": smfv.Ilu0Preconditioner(dA, K, reorder="multicolor"),
             "spmm": smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K), "X": torch.from_numpy(X).to(dev),
             "Y": torch.empty((m, K), dtype=torch.float64, device=dev), "W": torch.empty((m, K), dtype=torch.float64, device=dev)}
        copies.append(c)
    torch.cuda.synchronize()
    setup_s = time.time() - t0
    c0 = copies[0]
    Rd = c0["mc"].R
    i64 = lambda T: T.contiguous().view(torch.int64)  # noqa: E731
    same = lambda a, b: bool(torch.equal(i64(a), i64(b)))  # noqa: E731

    # ---- the bit-exactness checks, before anything is timed
    dX = c0["X"]
    perm_t = torch.from_numpy(Rd.perm.astype(np.int64)).to(dev)
    Xn = Rd.to_new(dX)
    checks = {"roundtrip": same(Rd.to_old(Xn), dX), "nt_equals_plain": same(Rd.to_new(dX, nt=True), Xn)
              and same(Rd.to_old(Xn, nt=True), dX), "to_new_equals_index_select": same(torch.index_select(dX, 0, perm_t), Xn)}
    pB = smfv.SpmmPlan(smfv.Variant.ROWWISE, Rd.B, K)
    YA = c0["spmm"].run(dX, torch.empty_like(dX))
    checks["B_Px_equals_P_Ax"] = same(pB.run(Xn, torch.empty_like(dX)), Rd.to_new(YA))
    Zmc, Znat = c0["mc"].apply(dX).clone(), c0["nat"].apply(dX).clone()
    checks["applies_finite"] = bool(torch.isfinite(Zmc).all()) and bool(torch.isfinite(Znat).all())
    checks["applies_differ"] = not same(Zmc, Znat)  # another preconditioner
    torch.cuda.synchronize()
    del pB
    if not all(checks.values()):
        print(json.dumps({"checks": checks}))
        raise SystemExit("reorder_ab: a bit-exactness check failed; nothing was timed")

    def step(form: str, i: int) -> None:
        c = copies[i % len(copies)]
        which, _, what = form.partition("_")
        if form == "spmm":
            c["spmm"].run(c["X"], c["Y"])
        elif form == "to_new":
            c["mc"].R.to_new(c["X"], c["Y"])
        elif form == "to_old":
            c["mc"].R.to_old(c["X"], c["Y"])
        elif what == "lower":
            c[which].lower.solve(c["X"], c["Y"])
        elif what == "upper":
            c[which].upper.solve(c["X"], c["Y"])
        elif what == "ilu0":
            c[which].plan.factor(c[which].F.values)
        elif what == "apply":
            c[which].apply(c["X"], c["Y"])
        elif what == "apply_nt":  # mc_apply with non-temporal stores in both permutations
            M = c["mc"]
            W = M.R.to_new(c["X"], M._w, nt=True)
            M.lower.solve(W, W)
            M.upper.solve(W, W)
            M.R.to_old(W, c["Y"], nt=True)
        elif what == "apply_noperm":
            c["mc"].lower.solve(c["X"], c["Y"])
            c["mc"].upper.solve(c["Y"], c["Y"])
        else:
            raise KeyError(form)

    names = ["nat_lower", "mc_lower", "nat_upper", "mc_upper", "nat_ilu0", "mc_ilu0", "nat_apply", "mc_apply",
             "mc_apply_nt", "mc_apply_noperm", "to_new", "to_old", "spmm"]
    st = {w: {"ilu0": c0[w].plan.stats(), "lower": c0[w].lower.stats(), "upper": c0[w].upper.stats()} for w in ("nat", "mc")}
    launches = {}
    for w in ("nat", "mc"):
        lo, up = st[w]["lower"]["launches"], st[w]["upper"]["launches"]
        launches.update({f"{w}_lower": lo, f"{w}_upper": up, f"{w}_ilu0": st[w]["ilu0"]["launches"], f"{w}_apply": lo + up})
    launches["mc_apply"] += 2
    launches["mc_apply_noperm"] = launches["mc_apply"] - 2
    launches["mc_apply_nt"] = launches["mc_apply"]
    steps = {f: max(2, min(args.max_steps, args.nodes // max(1, launches[f]))) for f in launches}
    steps.update({"to_new": 100, "to_old": 100, "spmm": 200})

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
        return e0.elapsed_time(e1) * 1e3 / nsteps  # us per execution

    graphs = {f: captured(lambda i, f=f: step(f, i), steps[f], max(2, len(copies))) for f in names}
    us = {f: [] for f in names}
    for _ in range(args.rounds):
        for f in names:
            us[f].append(round(timed(graphs[f], steps[f]), 2))
    med = {f: statistics.median(v) for f, v in us.items()}
    spread = {f: round((max(v) - min(v)) / med[f], 4) for f, v in us.items()}
    out = {
        "what": f"natural against multicolour ordering on the cop20k {args.matrix} stand-in, K = 32, us per execution (copies rotated)",
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "copies_rotated": len(copies), "m": m, "nnz": nnz,
        "symmetric": symmetric, "ncolors": Rd.ncolors, "setup_s": round(setup_s, 1), "checks": checks, "steps_per_graph": steps,
        "us": us, "median_us": med, "spread_over_median": spread,
        "levels": {w: {k: st[w][k]["levels"] for k in st[w]} for w in st},
        "launches": {w: {k: st[w][k]["launches"] for k in st[w]} for w in st},
        "speedup_nat_over_mc": {k: round(med[f"nat_{k}"] / med[f"mc_{k}"], 2) for k in ("lower", "upper", "ilu0", "apply")},
        "permutations_us": round(med["mc_apply"] - med["mc_apply_noperm"], 2),
        "permutations_share_of_apply": round((med["mc_apply"] - med["mc_apply_noperm"]) / med["mc_apply"], 4),
        "reorder_plan": Rd.stats(),
    }
    del graphs

    # ---- k_permute_rows against a copy of the same bytes and torch.index_select
    if args.matrix == "stencil" and not args.no_rows:
        nb = 6  # (X, Y) pairs rotated: 62 MB each
        Xs = [torch.from_numpy(X).to(dev) for _ in range(nb)]
        Ys = [torch.empty((m, K), dtype=torch.float64, device=dev) for _ in range(nb)]
        inv_t = torch.empty_like(perm_t)
        inv_t[perm_t] = torch.arange(m, device=dev)
        nbytes = m * K * 8

        def rows_fn(direction, nt):
            fn = Rd.to_new if direction == "to_new" else Rd.to_old
            return lambda i: fn(Xs[i % nb], Ys[i % nb], nt=nt)

        rforms = {"to_new_plain": rows_fn("to_new", False), "to_new_nt": rows_fn("to_new", True),
                  "to_old_plain": rows_fn("to_old", False), "to_old_nt": rows_fn("to_old", True),
                  "stream_copy": lambda i: call("smfv_stream_copy", Ys[i % nb].data_ptr(), Xs[i % nb].data_ptr(), nbytes,
                                                stream_handle(None)),
                  "index_select_to_new": lambda i: torch.index_select(Xs[i % nb], 0, perm_t, out=Ys[i % nb]),
                  "index_select_to_old": lambda i: torch.index_select(Xs[i % nb], 0, inv_t, out=Ys[i % nb])}
        rsteps = 120
        rgraphs = {f: captured(fn, rsteps, nb) for f, fn in rforms.items()}
        rus = {f: [] for f in rforms}
        for _ in range(args.rounds):
            for f in rforms:
                rus[f].append(round(timed(rgraphs[f], rsteps), 2))
        rmed = {f: statistics.median(v) for f, v in rus.items()}
        out["permute_rows"] = {
            "what": "k_permute_rows, m = 121,192, K = 32, us per call; bytes = read + written", "bytes": 2 * nbytes,
            "pairs_rotated": nb, "steps_per_graph": rsteps, "us": rus, "median_us": rmed,
            "spread_over_median": {f: round((max(v) - min(v)) / rmed[f], 4) for f, v in rus.items()},
            "TBps": {f: round(2 * nbytes / rmed[f] / 1e6, 3) for f in rmed},
            "ratio_to_stream_copy": {f: round(rmed[f] / rmed["stream_copy"], 3) for f in rmed}}
        del rgraphs, Xs, Ys

    # ---- what the weaker preconditioner costs: block PCG, per-column scalars
    if args.matrix == "stencil" and not args.no_pcg:
        dA, spmm = c0["A"], c0["spmm"]
        Bm = torch.from_numpy(rng.uniform(-1, 1, (m, K))).to(dev)
        bnorm = Bm.norm(dim=0)
        Q, Z = torch.empty_like(Bm), torch.empty_like(Bm)

        def pcg(M, iters=None):
            """iters None: until every column's relative residual is <= TOL (checked every iteration,
            a host read-back); else exactly `iters` iterations with no read-back, timed with events."""
            Xk, Rk = torch.zeros_like(Bm), Bm.clone()
            M.apply(Rk, Z)
            P = Z.clone()
            rz = (Rk * Z).sum(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            it = 0
            while it < (iters if iters is not None else args.max_iters):
                spmm.run(P, Q)
                alpha = rz / (P * Q).sum(0)
                Xk += alpha * P
                Rk -= alpha * Q
                it += 1
                if iters is None and float((Rk.norm(dim=0) / bnorm).max()) <= TOL:
                    break
                M.apply(Rk, Z)
                rz_new = (Rk * Z).sum(0)
                P = Z + (rz_new / rz) * P
                rz = rz_new
            e1.record()
            torch.cuda.synchronize()
            spmm.run(Xk, Q)
            true_rel = float(((Bm - Q).norm(dim=0) / bnorm).max())
            return it, e0.elapsed_time(e1) * 1e3 / max(1, it), true_rel

        res = {}
        for w in ("nat", "mc"):
            it, _, rel = pcg(c0[w])
            per = [round(pcg(c0[w], it)[1], 1) for _ in range(args.rounds)]
            res[w] = {"iterations": it, "true_relative_residual": rel, "us_per_iteration": per,
                      "median_us_per_iteration": statistics.median(per),
                      "ms_to_tolerance": round(it * statistics.median(per) / 1e3, 2)}
        out["pcg"] = {"what": f"block PCG in torch, K = {K} right-hand sides, relative residual {TOL}, per-column alpha / beta; "
                              "an iteration = A P (SpmmPlan), Ilu0Preconditioner.apply and torch's vector updates, eager launches",
                      "max_iters": args.max_iters, **res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
