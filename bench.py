#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X SpMM engine.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cop20k_k32] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times K steps as one region and prints the
result line (metric, value, unit, higher_is_better, dtype, ms_per_step).
--full adds everything measured beside that figure: the CPU baseline, nine
more timed regions (value is then their median), the bind / rebind, warm,
copy-floor and rocSPARSE legs, the plans timed beside a decomposed step and
the post-timing result check (exit status 3 when it fails).
--dump-outputs DIR writes the Y of the last timed step as DIR/Y.npy.

Metric (BASELINE.json): effective GFLOP/s (= 2*nnz*K / t, the reference's
own formula, results/visualisation_fat_vector.ipynb:1595-1601) and achieved
HBM GB/s, cop20k_A x K=32.  A step is one SpMM launch over one resident
problem; inputs are in HBM before the timed region starts.  The workload
rotates over enough copies of (A, X, Y) that every launch streams from HBM
rather than from the 256 MiB Infinity Cache (cold); the same-copy (warm)
rate is reported beside it.

N > 1 (one process per GPU).  Under torch.distributed.run (WORLD_SIZE set)
every process is one rank and --gpus must equal WORLD_SIZE; a plain
`python bench.py --gpus N` starts the N ranks itself, as children
(torch.distributed.run on 127.0.0.1, no exec), and re-prints rank 0's line --
the reference's `mpirun -np P ./prog` (SC/scripts/mpi.sub:97).  ONE problem
decomposed over the ranks as the reference's RowWise does
(SC/...RowWise.cpp:26-29): each rank runs its row block (a tiled plan where
the pattern re-uses X rows), then one RCCL all-gather of the Y blocks over
xGMI (the reference's MPI_Gatherv, :85-87) -> strong scaling; value = the
problem's flops / the max-over-ranks time of (kernel + exchange).  The
rank-local kernel time and the exchange are reported separately, and the
independent-copy rate (every rank its own whole problem, no collective) as a
secondary field.  --mode replicas makes that the value instead.

cop20k_A.mtx (SuiteSparse) is not available offline: unless --mtx points at
it, the matrix is the labelled surrogate of inputs.cop20k_surrogate() (same
m = 121,192, nnz = 2,624,346 vs 2,624,331, symmetric 27-point-stencil
pattern).  X is the reference's fat vector (rand()%100+1, glibc seed 1).

The cpu_baseline leg (rank 0, before the GPU is touched; r6: at every N,
the other ranks waiting in the rendezvous) times the REFERENCE's own RowWise
MPI kernel (oracle/_ref/ref_driver, its sources compiled unmodified) under
mpiexec on the host cores, as SC/main.cpp:161-163 times it -- 16 ranks at
N = 1 (with a 1-16 sweep), 16 * N ranks beside an N-GPU line; without that
binary it falls back to the oracle's C port.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HEADLINE_METRIC = "effective GFLOP/s + achieved HBM GB/s, cop20k_A × K=32, 1/2/4/8 GPUs"


def metric_for(config: str, K: int, variant: str) -> str:
    """BASELINE.json's metric on its headline config; the same quantities,
    labelled with the config actually run, on the others."""
    if config == "cop20k_k32" and variant == "ROWWISE":
        return HEADLINE_METRIC
    what = {"cop20k": "cop20k_A", "pow10m": "synthetic 10M x 10M power-law", "syn80m": "synthetic 80M x 80M",
            "cop20k_perm": "cop20k_A (randomly permuted)",
            "cop20k_irr": "cop20k_A (irregular surrogate)"}[CONFIGS[config][0]]
    return f"effective GFLOP/s + achieved HBM GB/s, {what} × K={K}, {variant}"


STABILIZE_REPLAYS_COLLECTIVE = 10  # the same, as a count every rank replays (graphs with RCCL calls)
STABILIZE_S = 0.1  # untimed graph replays before the first timed region (clock ramp)
GRAPH_CHUNK = 4096  # most launches captured into one hipGraph; a longer timed region replays it
DUMP_LIMIT_BYTES = 64_000_000  # --dump-outputs: most bytes written in all
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
MPIEXEC = "/opt/conda/bin/mpiexec"

CONFIGS = {
    # name: (matrix, K, variant)
    "cop20k_k32": ("cop20k", 32, "ROWWISE"),
    "cop20k_k128": ("cop20k", 128, "ROWWISE"),
    "cop20k_k1": ("cop20k", 1, "SEQUENTIAL"),
    "pow10m_k32": ("pow10m", 32, "NONZERO"),
    "pow10m_k1": ("pow10m", 1, "SEQUENTIAL"),  # K = 1 on power-law rows (k_spmv_stream long rows)
    # the headline matrix under a random symmetric permutation (ordering robustness)
    "cop20k_perm_k32": ("cop20k_perm", 32, "ROWWISE"),
    # a second cop20k_A stand-in with the same m and nnz, unstructured (k-NN of
    # clustered 3-D points, row degrees 4..85): the plan on an irregular pattern
    "cop20kirr_k32": ("cop20k_irr", 32, "ROWWISE"),
    "cop20kirr_k1": ("cop20k_irr", 1, "SEQUENTIAL"),
    # config 5: 80M x 80M, 16 nnz/row, row-partitioned over the ranks + RCCL all-gather
    "syn80m_k32": ("syn80m", 32, "ROWWISE"),
}
SYN80M_ROWS = 80_000_000


def measured_traffic(config: str, kernel: str):
    """Per-launch HBM bytes of this config's kernel from the committed
    rocprofv3 PMC run (profiles/pmc_traffic.json, scripts/pmc_traffic.py)."""
    import json as _json
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        e = _json.load(open(path)).get(config)
    except (OSError, ValueError):
        return None, None
    if not e or kernel.split("<")[0] not in (e.get("kernel") or ""):
        return None, None
    return e["traffic_bytes_per_launch"], e["source"]


def lds_staged_bytes(st: dict, K: int):
    """(r6) Bytes a k_rows_ws plan moves into LDS per launch: every tile's X
    union once per 32-column panel (staged_rows * 8 K), plus its meta once
    (values snapshot 8 B + u8 offset 1 B per entry, 1 KiB record per tile).
    Mostly L2 / MALL hits: the HBM side is roofline.traffic."""
    if st.get("kernel") != "k_rows_ws" or not st.get("tiled"):
        return None
    x = st["staged_rows"] * 8 * K
    meta = st["snapshot_entries"] * 9 + st["tiles"] * 1024
    return {"x_images": int(x), "meta": int(meta), "total": int(x + meta)}


def measured_rank_traffic(config: str, p: int, rank: int, kernel: str):
    """(r6) Per-launch HBM bytes of rank `rank`'s plan of the p-rank
    decomposition (profiles/pmc_traffic.json key '<config>@p<p>r<rank>',
    from a PMC run of `bench.py --rank-plans p --rank-only rank`: the same
    rank plan smfv_dist_plan_create gives that rank)."""
    if p == 1:  # one rank: its plan is the whole matrix's (the N = 1 line's traffic)
        return measured_traffic(config, kernel)
    return measured_traffic(f"{config}@p{p}r{rank}", kernel)


def kernel_label(variant: str, K: int, plan_stats: dict, x_bytes: int = 0) -> str:
    if variant == "NONZERO" and not plan_stats.get("tiled"):
        return "k_merge_flat + k_carry_fixup" if K % 32 == 0 else "k_merge + k_carry_fixup"
    if plan_stats.get("mfma"):
        return "k_rows_mfma"
    if plan_stats.get("kernel"):
        return plan_stats["kernel"]
    if plan_stats.get("tiled"):
        return "k_spmv_chunks" if K == 1 else "k_rows_ws"
    if K == 1:
        return "k_spmv_stream<256, 64, 2048>"
    if K % 2:
        return "k_rows<TEAM,1>"
    pairs = K // 2
    cfg = (16, 4, 4) if pairs >= 64 else (8, 2, 8) if pairs >= 16 else (8, 1, 8) if pairs >= 8 else \
        (4, 1, 8) if pairs >= 4 else (2, 1, 8) if pairs >= 2 else (1, 1, 8)
    buf = "true" if 0 < x_bytes <= 0x7FFFFFFF else "false"  # buffer-resource X gathers when X < 2 GiB
    return "k_rows_mh<%d, %d, %d, %s>" % (cfg + (buf,))


def algorithmic_bytes(m: int, n: int, nnz: int, K: int) -> int:
    """CSR read once + X read once + Y written once."""
    return 12 * nnz + 4 * (m + 1) + 8 * n * K + 8 * m * K


def build_matrix(kind: str, mtx: str | None):
    from sparsematrixmultiplicationmpi_amd import inputs
    if mtx:
        return inputs.readMatrixMarketFile(mtx), f"{os.path.basename(mtx)}"
    if kind == "cop20k":
        return inputs.cop20k_surrogate(), "cop20k_A surrogate (fem27, m=121192, symmetric)"
    if kind == "cop20k_perm":
        import numpy as np
        A = inputs.cop20k_surrogate()
        perm = np.random.default_rng(2024).permutation(A.numRows)
        return (inputs.permute_symmetric(A, perm),
                "cop20k_A surrogate under a random symmetric permutation (seed 2024)")
    if kind == "cop20k_irr":
        return (inputs.cop20k_irregular_surrogate(),
                "cop20k_A irregular surrogate (knn3d: clustered 3-D points, variable-k nearest neighbours, "
                "symmetrised, Morton order; m=121192, degrees 4..85)")
    if kind == "pow10m":
        m = 10_000_000
        return (inputs.gen_random_rows(m, m, 16.0, 2.0, 4096, 42),
                "synthetic 10M x 10M power-law rows (alpha 2, cap 4096, mean 16)")
    raise ValueError(kind)


# ---------------------------------------------------------------------------
# CPU baseline (reference RowWise under MPI on the host cores)
# ---------------------------------------------------------------------------
MPI_BIND = ["-bind-to", "core"]  # (r4) one rank per core, stated in cpu_baseline.binding


def _ref_run(A, K: int, tag: str, cores: int, binary: str, reps: int, timeout: float) -> float | None:
    """One timed run of the reference's compiled sources (oracle/_ref) under
    MPICH: seconds per call of variant `tag`, as SC/main.cpp:161-163 times it."""
    from sparsematrixmultiplicationmpi_amd import inputs
    name = {"R": "Row-wise", "C": "Column-wise", "Z": "Non-zero Elements", "S": "Serial Algo"}[tag]
    with tempfile.TemporaryDirectory() as tmp:
        csr = os.path.join(tmp, "a.bin")
        inputs.write_csr_bin(csr, A)
        cmd = [MPIEXEC, "-launcher", "fork"] + MPI_BIND + ["-n", str(cores), binary, csr, str(K), "--reps",
                                                            str(reps), "--variants", tag]
        # own process group: on a timeout mpiexec AND its ranks are killed
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                start_new_session=True)
        try:
            out, err = proc.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            import signal
            os.killpg(proc.pid, signal.SIGKILL)
            proc.communicate()
            print(f"[bench] reference CPU run over {timeout:.0f} s (-n {cores}); killed", file=sys.stderr)
            return None
        if proc.returncode != 0:
            print(f"[bench] reference CPU run failed (rc {proc.returncode}): {err[-300:]}", file=sys.stderr)
            return None
    mt = re.search(rf"{re.escape(name)} Execution time: ([0-9.eE+-]+)", out)
    return float(mt.group(1)) if mt else None


def cpu_ranks(world: int) -> int:
    """MPI ranks of the CPU baseline beside an N-GPU line: 16 per GPU (the
    box's CPU share of one GPU), capped at the CPUs this process may use
    when N > 1 (N = 1 keeps the 16-rank point and its 1-16 sweep)."""
    if world <= 1:
        return 16
    return max(1, min(16 * world, len(os.sched_getaffinity(0))))


def cpu_baseline(A, K: int, variant: str, sample: str | None = None, budget_s: float = 20.0,
                 sweep_ranks: bool = True, ranks: int = 16) -> dict:
    """The reference's own kernel (its sources compiled unmodified, g++ -O3,
    oracle/_ref/ref_driver) under mpiexec on this box's host cores: the
    16-rank rate (the box's CPU share per GPU) is `value`;
    `sweep_GFLOPs_by_ranks` holds 1/2/4/8/16 ranks and `O0_GFLOPs` the
    16-rank rate of the reference's documented unoptimised compile
    (README.md:29).  `sample` labels a bounded stand-in input
    (configs 4-5).  (r6) `ranks` != 16 (an N-GPU line: 16 * N, cpu_ranks)
    times that many ranks as `value`, with the 16-rank point beside it, and
    no sweep.  Without the binary: the oracle's C port, one thread."""
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    ref0 = ref + "_O0"
    flops = 2.0 * A.nnz * K
    tag = {"ROWWISE": "R", "COLUMNWISE": "C", "NONZERO": "Z", "SEQUENTIAL": "S"}[variant]
    name = {"R": "Row-wise", "C": "Column-wise", "Z": "Non-zero Elements", "S": "Serial Algo"}[tag]
    what = sample or f"full matrix, K={K}"
    if os.path.exists(ref) and os.path.exists(MPIEXEC):
        t0 = time.time()
        # 16 = this process's CPU share on the GPU box (gpurun: 16 per GPU);
        # SURVEY 8(d) also asks for -n nproc: run last, capped in time (over
        # the share it oversubscribes the 16 CPUs; its rate is reported, not used)
        nproc = os.cpu_count() or 16
        if tag == "S":
            counts = [1]
        elif ranks != 16:
            sweep_ranks = False
            counts = sorted({min(16, ranks), ranks})
        else:
            counts = [1, 2, 4, 8, 16] if sweep_ranks else [16]
        many = len(counts) > 1
        sweep = {}
        for c in counts:
            # the reported point (the top rank count): median of 10 calls
            t = _ref_run(A, K, tag, c, ref, 10 if c == counts[-1] else 3, budget_s * 6)
            if t:
                sweep[str(c)] = round(flops / t / 1e9, 4)
        nproc_point = None
        if sweep_ranks and tag != "S" and nproc not in counts:
            t = _ref_run(A, K, tag, nproc, ref, 3, 30.0)
            nproc_point = {"ranks": nproc, "GFLOPs": round(flops / t / 1e9, 4) if t else None,
                           "note": "mpiexec -n nproc (SURVEY 8d); nproc counts the whole host, this process's "
                                   "share is 16 CPUs, so it oversubscribes; None = over its 30 s cap or failed"}
        top = str(counts[-1])
        if top in sweep:
            o0 = (_ref_run(A, K, tag, counts[-1], ref0, 3, budget_s * 6)
                  if os.path.exists(ref0) and sweep_ranks else None)
            return {"value": sweep[top], "unit": "GFLOP/s", "cores": counts[-1], "kind": "reference",
                    "host_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
                    "binding": "MPICH hydra " + " ".join(MPI_BIND) + " (one rank per core), -launcher fork",
                    "nproc_point": nproc_point,
                    "sample": f"{what}, reference {name} (SC sources, g++ -O3) under MPICH mpiexec -n {top}, "
                              f"median of 10 calls incl. gather + FatVector rebuild"
                              f"{'; 1/2/4/8/16-rank sweep and the -O0 build beside it' if sweep_ranks else ''}"
                              f"{'; the 16-rank point (one GPU share) beside it' if many and not sweep_ranks else ''}; "
                              f"wall {time.time() - t0:.1f}s",
                    "seconds_per_call": flops / (sweep[top] * 1e9),
                    "sweep_GFLOPs_by_ranks": sweep,
                    "O0_GFLOPs": round(flops / o0 / 1e9, 4) if o0 else None}
    # fallback: the oracle's C restatement, one thread
    from sparsematrixmultiplicationmpi_amd import inputs
    from oracle import oracle
    X = inputs.generateLargeFatVector(A.numCols, K)
    t0 = time.perf_counter()
    oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    t = time.perf_counter() - t0
    return {"value": round(flops / t / 1e9, 4), "unit": "GFLOP/s", "cores": 1, "kind": "port",
            "sample": f"{what}, oracle C restatement (sequential), one call", "seconds_per_call": t}


def stream_copy_gbps(dev, nbytes: int = 2 << 30, reps: int = 5) -> float:
    """Measured HBM copy rate on this GPU (read + write bytes / time of a
    2 GiB copy by the library's 16-byte non-temporal copy kernel,
    smfv_stream_copy): the practical ceiling next to the 8 TB/s spec that
    roofline.peak quotes ('measure a STREAM-copy peak')."""
    import torch
    from sparsematrixmultiplicationmpi_amd._lib import call
    a = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    a.fill_(1.0)
    st = torch.cuda.current_stream().cuda_stream
    call("smfv_stream_copy", b.data_ptr(), a.data_ptr(), nbytes, st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call("smfv_stream_copy", b.data_ptr(), a.data_ptr(), nbytes, st)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * nbytes / (ms * 1e-3) / 1e9


def size_matched_copy(dev, prob_bytes: int, ncopies: int, steps: int, world: int) -> dict | None:
    """The launch-size floor beside the spec: the same 16-byte non-temporal
    copy kernel moving the SpMM's algorithmic bytes per launch (half read,
    half written), rotated over as many buffer pairs as the SpMM's cold
    copies and timed the same way (one graph of `steps` launches).  Start-up
    and drain of a ~100 MB launch are in it, as they are in the SpMM's.
    None where the rotation would not fit comfortably (> 8 GiB)."""
    import torch
    from sparsematrixmultiplicationmpi_amd._lib import call
    half = (prob_bytes // 2) // 16 * 16
    if half <= 0 or ncopies * 2 * half > (8 << 30):
        return None
    bufs = [(torch.empty(half // 8, dtype=torch.float64, device=dev),
             torch.empty(half // 8, dtype=torch.float64, device=dev)) for _ in range(ncopies)]
    for a, _ in bufs:
        a.fill_(1.0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = torch.cuda.current_stream().cuda_stream
            for i in range(steps):
                a, b = bufs[i % ncopies]
                call("smfv_stream_copy", b.data_ptr(), a.data_ptr(), half, st)
    torch.cuda.current_stream().wait_stream(side)
    _stabilize(g)
    ms = _timed_events(g.replay, world) / steps
    del g, bufs
    torch.cuda.empty_cache()
    return {"bytes_per_launch": 2 * half, "avg_launch_ms": round(ms, 6),
            "GBps": round(2 * half / (ms * 1e-3) / 1e9, 1),
            "note": "smfv_stream_copy of the algorithmic bytes per launch, cold rotation, one graph of the "
                    "timed step count; frac_of_copy_time = copy time / SpMM time"}


def mix_matched_copy(dev, rbytes: int, wbytes: int, ncopies: int, steps: int, world: int) -> dict | None:
    """(r6, VERDICT r5 #2a) The floor of the SpMM's own byte MIX: it reads ~2
    bytes (CSR + X) per byte written (Y), where size_matched_copy is 1:1.
    smfv_stream_mix moves the SpMM's algorithmic read and write bytes per
    launch under the same rotation and timing, three ways: `plain` (each lane
    reads 32 B non-temporally and writes their 16-B sum), and `lds32` /
    `lds64` (k_rows_ws's pipeline shape: 1024-lane block per CU, loader waves
    LDS-DMA units of 32 / 64 KiB into two LDS slots, writer waves store from
    LDS, one barrier per unit; lds32 runs ~7.5 units per CU, the headline
    plan's 7.9).  None where the rotation would not fit (> 8 GiB)."""
    import torch
    from sparsematrixmultiplicationmpi_amd._lib import call
    w = (wbytes // 16) * 16
    r = 2 * w  # the plain probe reads exactly 2x; the LDS probes take the real read bytes below
    rr = (rbytes // 16) * 16
    if w <= 0 or ncopies * (max(r, rr) + w) > (8 << 30):
        return None
    bufs = [(torch.empty(max(r, rr) // 8, dtype=torch.float64, device=dev),
             torch.empty(w // 8, dtype=torch.float64, device=dev)) for _ in range(ncopies)]
    for a, _ in bufs:
        a.fill_(1.0)
    out = {"read_bytes_per_launch": rr, "write_bytes_per_launch": w,
           "note": "smfv_stream_mix, cold rotation over the SpMM's copy count, one graph of the timed step count; "
                   "plain reads 2x the write bytes (32 B per 16 B written); frac_of_spmm_time = probe / SpMM time"}
    for name, unit, nread in (("plain", 0, r), ("lds32", 32, rr), ("lds64", 64, rr)):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                st = torch.cuda.current_stream().cuda_stream
                for i in range(steps):
                    a, b = bufs[i % ncopies]
                    call("smfv_stream_mix", b.data_ptr(), w, a.data_ptr(), nread, unit, st)
        torch.cuda.current_stream().wait_stream(side)
        _stabilize(g)
        ms = _timed_events(g.replay, world) / steps
        del g
        out[name] = {"avg_launch_ms": round(ms, 6), "bytes_per_launch": nread + w,
                     "GBps": round((nread + w) / (ms * 1e-3) / 1e9, 1)}
    del bufs
    torch.cuda.empty_cache()
    return out


def _stabilize(g) -> int:
    """Untimed replays of a captured graph for >= STABILIZE_S before its first
    timed region: the GPU's clocks ramp over ~10 ms of load, and one warm
    replay (~5 ms at the headline) left the first timed region ~6 % slower
    than every later one (r2 samples: 25.76 us vs a 24.16 us median).
    Returns the number of replays."""
    import torch
    t_end = time.time() + STABILIZE_S
    reps = 0
    while reps < 2 or (time.time() < t_end and reps < 200):
        g.replay()
        torch.cuda.synchronize()
        reps += 1
    return reps


def vendor_leg(copies, steps: int, timed, flops: float):
    """rocSPARSE generic SpMM (the PETSc-block analogue, SC/main.cpp:289-402)
    on the same resident copies, same rotation and graph timing as the
    engine's kernel: the library line beside `value`, not part of it."""
    import torch
    import sparsematrixmultiplicationmpi_amd as smfv
    try:
        vs = torch.cuda.Stream()  # rocSPARSE launches on the stream bound at creation: capture on it
        hs = [smfv.VendorSpmm(plan.A, dX, dY, alg=0, stream=vs) for plan, dX, dY in copies]
        with torch.cuda.stream(vs):
            for h in hs:
                h.run()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=vs):
            for i in range(steps):
                hs[i % len(hs)].run()
        _stabilize(g)
        ms = timed(g) / steps
        return {"library": "rocSPARSE rocsparse_spmm (CSR, f64, row-major, alg default)",
                "avg_launch_ms": round(ms, 6), "GFLOPs": round(flops / (ms * 1e-3) / 1e9, 3),
                "timing": "same copies / rotation / hipGraph replay as the engine's kernel"}
    except Exception as e:  # a comparator must never sink the headline line
        return {"library": "rocSPARSE", "error": repr(e)[:200]}


# ---------------------------------------------------------------------------
# sampled result check (configs whose full reference result is too large)
# ---------------------------------------------------------------------------
def sampled_check(A, rows, dX, Ydev, exact: bool, row_base: int = 0) -> dict:
    """Recompute the sampled rows on the host in the reference's order (per
    row, non-zeros ascending, y += a * x with separate multiply and add:
    SC/SparseMatrixFatVectorMultiply.cpp:17-27) and compare with the
    device result: bit for bit (exact) or within 1e-12 x sum|a||x|
    (NONZERO's reassociated sums).  rows are A's local rows; Ydev row
    (row - row_base) holds row `row`.  Runs after the timed region."""
    import numpy as np
    import torch
    from sparsematrixmultiplicationmpi_amd import sampling
    t0 = time.time()
    srp, scol, sval, ucols = sampling.sub_csr(A.rowPtr, A.colIndices, A.values, rows)
    Xs = dX[torch.from_numpy(ucols).to(dX.device)].cpu().numpy()
    K = Xs.shape[1]
    lens = np.diff(srp.astype(np.int64))
    acc = np.zeros((len(rows), K))
    scale = np.zeros((len(rows), K))
    for j in range(int(lens.max()) if len(lens) else 0):  # position j of every row, in CSR order
        live = np.flatnonzero(lens > j)
        e = srp[live].astype(np.int64) + j
        prod = sval[e][:, None] * Xs[scol[e]]
        acc[live] = acc[live] + prod
        scale[live] = scale[live] + np.abs(prod)
    Ys = Ydev[torch.from_numpy(np.asarray(rows) - row_base).to(Ydev.device)].cpu().numpy()
    if exact:
        ok = bool(np.array_equal(Ys.view(np.uint64), acc.view(np.uint64)))
        err = float(np.max(np.abs(Ys - acc))) if len(rows) else 0.0
    else:
        rel = np.abs(Ys - acc) / np.maximum(scale, 1e-300)
        err = float(rel.max()) if len(rows) else 0.0
        ok = bool(err <= 1e-12)
    return {"rows_checked": int(len(rows)), "ok": ok, "max_err": err,
            "criterion": "bit-identical" if exact else "|y - y_ref| <= 1e-12 x sum|a||x|",
            "sample": "longest rows, merge-team boundary (carry) rows, empty, first/last, random",
            "seconds": round(time.time() - t0, 1)}


def dump_outputs(path: str, Y) -> None:
    """--dump-outputs DIR: the Y of the last timed step as DIR/Y.npy (float64),
    whole when it fits DUMP_LIMIT_BYTES, else a fixed sample of its rows
    (seed 0, ascending), so two builds given the same arguments write
    arrays that compare element for element."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    keep = (DUMP_LIMIT_BYTES - 1024) // (8 * Y.shape[1])  # (1 KiB: the .npy header)
    if Y.shape[0] > keep:
        rows = np.sort(np.random.default_rng(0).choice(Y.shape[0], keep, replace=False))
        Y = Y[torch.from_numpy(rows).to(Y.device)]
    np.save(os.path.join(path, "Y.npy"), Y.to(torch.float64).cpu().numpy())


class Deadline:
    """Per-phase watchdog for the multi-GPU paths: if a phase (communicator
    set-up, plan creation, warm-up, timing, check) runs past its limit -- an
    RCCL call that never returns on a first 8-GPU run -- the watchdog prints
    one diagnostic JSON line naming the phase and ends the process with exit
    status 4, so the driver gets a line and a status instead of a timeout.
    A ctypes / HIP call releases the GIL, so the watchdog thread runs while
    the main thread is stuck in one."""

    def __init__(self, seconds: float, rank: int, world: int, metric: str):
        self.seconds, self.rank, self.world, self.metric = seconds, rank, world, metric
        self.timer = None
        self.phase = None

    def enter(self, phase: str, seconds: float | None = None) -> None:
        import threading
        self.cancel()
        self.phase = phase
        if self.seconds <= 0:
            return
        limit = self.seconds if seconds is None else seconds
        t0 = time.time()

        def expire():
            print(json.dumps({"metric": self.metric, "value": None, "unit": "GFLOP/s", "n_gpus": self.world,
                              "error": f"rank {self.rank}: phase '{phase}' exceeded its {limit:.0f} s "
                                       f"deadline ({time.time() - t0:.0f} s)", "rank": self.rank}), flush=True)
            print(f"[bench] rank {self.rank}: deadline in phase {phase}; exiting with status 4",
                  file=sys.stderr, flush=True)
            os._exit(4)
        self.timer = threading.Timer(limit, expire)
        self.timer.daemon = True
        self.timer.start()

    def cancel(self) -> None:
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None


def _timed_events(fn, world: int):
    """HIP events on the current stream around fn(), bracketed by a barrier +
    synchronize on both sides (max over ranks is taken by the caller)."""
    import torch
    import torch.distributed as dist
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    return e0.elapsed_time(e1)


def _graph_or_eager(step, steps: int, world: int):
    """Time `steps` calls of step(i): captured into one hipGraph and replayed
    (RCCL calls included) when capture works, else launched eagerly.
    Returns (ms per step, how)."""
    import torch
    import torch.distributed as dist
    g, err = None, None
    try:
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(steps):
                    step(i)
        torch.cuda.current_stream().wait_stream(side)
    except Exception as e:  # capture refused (e.g. a collective that cannot be captured)
        g, err = None, e
    torch.cuda.synchronize()
    if world > 1:  # every rank replays, or none does (the graph holds collectives)
        ok = torch.tensor([0.0 if g is None else 1.0], dtype=torch.float64)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if ok.item() == 0.0:
            g = None
    if g is not None:
        for _ in range(STABILIZE_REPLAYS_COLLECTIVE):  # a fixed count: the graph holds collectives
            g.replay()
        torch.cuda.synchronize()
        return _timed_events(g.replay, world) / steps, "hipGraph replay"
    print(f"[bench] graph capture failed here or on another rank ({err!r:.120}); timing eager launches",
          file=sys.stderr)
    for i in range(3):
        step(i)

    def run():
        for i in range(steps):
            step(i)
    return _timed_events(run, world) / steps, "eager launches"


CPU_BASELINE_WAIT_S = 900.0  # the other ranks' wait while rank 0 times the CPU baseline (N > 1)


def rendezvous_seconds(args, world: int) -> float:
    """Deadline of the process-group rendezvous: the ranks other than 0 wait
    there while rank 0 times the CPU baseline (N > 1)."""
    extra = CPU_BASELINE_WAIT_S if world > 1 and not args.no_cpu_baseline else 0.0
    return args.phase_timeout + extra


def rank0_cpu_baseline(args, world: int, rank: int, dl, fn):
    """(r6) The CPU/MPI baseline beside EVERY line, N > 1 included
    (north_star: GFLOP/s at 1/2/4/8 GPUs alongside the CPU/MPI baseline):
    rank 0 runs fn() -- the reference's kernel under mpiexec on 16 ranks per
    GPU (cpu_ranks) -- before anything touches a GPU, while the other ranks
    wait for it in the process-group rendezvous (under a longer deadline).
    Returns the baseline dict on rank 0, None elsewhere."""
    if args.no_cpu_baseline:
        return None
    if rank != 0:
        if world > 1 and dl is not None:
            dl.enter("waiting for rank 0's CPU baseline (process-group rendezvous)",
                     seconds=args.phase_timeout + CPU_BASELINE_WAIT_S)
        return None
    if dl is not None:
        dl.enter("CPU baseline (reference kernel under mpiexec, before the GPU is touched)",
                 seconds=args.phase_timeout + CPU_BASELINE_WAIT_S)
    cpu = fn()
    if cpu is not None and world > 1:
        cpu["note_n_gpus"] = (f"beside the {world}-GPU line: {cpu.get('cores')} MPI ranks (16 per GPU = "
                              f"{16 * world}, capped at the {len(os.sched_getaffinity(0))} CPUs this process may use)")
    return cpu


def bench_rowpart(args, world: int, rank: int, local: int, K: int) -> None:
    """BASELINE config 5: synthetic m x m (m = 80M), 16 uniform-random
    columns per row (splitmix64, seed 42), X = hash integers 1..100 (seed 43).
    Rank r generates ONLY its rows of the RowWise partition
    (SC/...RowWise.cpp:26-29) and holds X (n x K, 20.5 GB) replicated and
    Y (m x K) whole; a step = its row-block SpMM + the RowWise exchange as
    one ncclAllGather of the equal Y blocks over xGMI (a row-partitioned
    distributed plan, smfv_dist_plan_create_rowpart).  The problem is fixed
    as N grows (strong scaling).  After timing, a row sample is checked bit
    for bit against a host recomputation (rank 0: its own rows plus rows of
    every other rank's block, regenerated alone)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import dist as D
    from sparsematrixmultiplicationmpi_amd import inputs, sampling

    m = n = args.rows or SYN80M_ROWS
    dl = Deadline(args.phase_timeout, rank, world, metric_for("syn80m_k32", K, "ROWWISE"))

    def _cpu():
        # before the GPU is touched; the reference's int32 m*K indexing cannot
        # hold 80M x 32, so a bounded 1M x 1M instance of the same generator
        S = inputs.gen_random_rows(1_000_000, 1_000_000, 16.0, 0.0, 16, 42)
        return cpu_baseline(S, K, "ROWWISE", sample=f"bounded sample: 1M x 1M instance of the same generator "
                                                    f"(16 uniform-random columns per row), K={K}", sweep_ranks=False,
                            ranks=cpu_ranks(world))
    cpu = rank0_cpu_baseline(args, world, rank, dl, _cpu)
    first, last, _, _ = D.exchange_plan(smfv.Variant.ROWWISE, m, 0, None, K, world)
    r0, r1 = int(first[rank]), int(last[rank]) + 1
    t0 = time.time()
    A = inputs.gen_random_rows(m, n, 16.0, 0.0, 16, 42, r0, r1)
    t_gen = time.time() - t0
    nnz_loc = A.nnz
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    dl.enter("process group + RCCL communicator", seconds=rendezvous_seconds(args, world))
    if world > 1:
        dist.init_process_group("gloo")
    comm = D.Communicator.from_torch_distributed()
    rccl_n = comm.nranks()  # the ranks RCCL itself counts (ncclCommCount), reported as n_gpus
    ndevs = _devices_used(dev, world)
    dl.enter("inputs + plan")
    dA = smfv.DeviceCSR(A, dev)
    X = torch.empty((n, K), dtype=torch.float64, device=dev)
    smfv.fill_x_hash(X, 43)
    Y = torch.empty((m, K), dtype=torch.float64, device=dev)
    t0 = time.time()
    plan = D.DistPlan(comm, smfv.Variant.ROWWISE, dA, K, to_all=True, rowpart=True, m=m)
    torch.cuda.synchronize()
    t_plan = time.time() - t0
    dl.enter("warm-up (first collective: RCCL connection set-up)")
    for _ in range(max(args.warmup, 1)):  # (the first collective sets up RCCL's connections)
        plan.run(X, Y)
    torch.cuda.synchronize()
    # eager (the step holds an RCCL collective); ~65 ms per step at N = 1
    dl.enter("timed steps")
    ms_step = _timed_events(lambda: [plan.run(X, Y) for _ in range(args.steps)], world) / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, Y)
    # --full: the rank-local kernel alone, and the reference's own exchange
    # semantics beside the step: Gatherv to rank 0 (SC/...RowWise.cpp:85-87)
    # instead of the all-gather
    ms_kern = ms_root = 0.0
    if args.full:
        ms_kern = _timed_events(lambda: [plan.run_local(X, Y) for _ in range(args.steps)], world) / args.steps
        plan_root = D.DistPlan(comm, smfv.Variant.ROWWISE, dA, K, to_all=False, rowpart=True, m=m)
        plan_root.run(X, Y)
        ms_root = _timed_events(lambda: [plan_root.run(X, Y) for _ in range(args.steps)], world) / args.steps
        del plan_root
        # sampled check, outside the timed region: rank 0's rows + rows of the other blocks
        dl.enter("result check")
        plan.run(X, Y)
        torch.cuda.synchronize()
    chk = None
    if args.full and rank == 0:
        rows = sampling.sample_rows(A.rowPtr, K, n_random=2000)
        chk = sampled_check(A, rows, X, Y, exact=True, row_base=-r0)
        other_ok, other_n = True, 0
        for r in range(1, world):
            for g in np.random.default_rng(r).integers(int(first[r]), int(last[r]) + 1, 16):
                B = inputs.gen_random_rows(m, n, 16.0, 0.0, 16, 42, int(g), int(g) + 1)
                c = sampled_check(B, np.array([0]), X, Y, exact=True, row_base=-int(g))
                other_ok &= c["ok"]
                other_n += 1
        chk["other_blocks_rows_checked"], chk["ok"] = other_n, chk["ok"] and other_ok
    t = torch.tensor([ms_step, ms_kern, float(nnz_loc), ms_root], dtype=torch.float64)
    if world > 1:
        tn = torch.tensor([float(nnz_loc)], dtype=torch.float64)
        dist.all_reduce(tn)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        nnz_tot = int(tn.item())
    else:
        nnz_tot = nnz_loc
    dl.cancel()
    ms_step, ms_kern, ms_root = float(t[0]), float(t[1]), float(t[3])
    mloc = r1 - r0
    flops = 2.0 * nnz_tot * K
    kbytes = 12 * nnz_loc + 4 * (mloc + 1) + 8 * n * K + 8 * mloc * K  # rank 0's block, X read once
    gather_bytes = kbytes + 8 * nnz_loc * K  # random columns: one X row gathered per non-zero
    if rank == 0:
        out = {
            "metric": metric_for("syn80m_k32", K, "ROWWISE"),
            "value": round(flops / (ms_step * 1e-3) / 1e9, 3), "unit": "GFLOP/s",
            "n_gpus": rccl_n, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "ranks": {"rccl_nranks": rccl_n, "processes": world, "distinct_devices": ndevs},
            "data": f"synthetic: {m}x{m}, 16 uniform-random columns/row (splitmix64 seed 42), X hash 1..100 (seed 43)",
            "config": {"workload": f"syn80m_k32: {m}x{m} x K={K}, ROWWISE row-partitioned over {world} GPU(s)"
                                   " + RCCL all-gather of Y", "m": m, "n": n, "nnz": nnz_tot, "K": K,
                       "variant": "ROWWISE", "parallelism": f"rows/{world}, X replicated, Y all-gathered"},
            # (the rank-local kernel is timed alone, and the gather to rank 0, under --full)
            "roofline": {"bound": "hbm", "achieved": round(kbytes / (ms_kern * 1e-3) / 1e9, 1),
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(kbytes / (ms_kern * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "traffic": None,
                         "kernel": kernel_label("ROWWISE", K, plan.stats(), 8 * n * K),
                         "algorithmic_bytes_per_launch": kbytes,
                         "gather_model_GBps": round(gather_bytes / (ms_kern * 1e-3) / 1e9, 1),
                         "avg_launch_ms": round(ms_kern, 4),
                         "timing": "HIP events around eager launches (rank-local kernel alone; max over ranks)"}
            if args.full else None,
            "exchange_ms": round(ms_step - ms_kern, 4) if args.full else None,
            "exchange_ms_gather_to_root": round(ms_root - ms_kern, 4) if args.full else None,
            "exchange_note": "exchange_ms: all-gather of the Y blocks to every rank (ncclAllGather); "
                             "exchange_ms_gather_to_root: the reference's MPI_Gatherv semantics (grouped "
                             "ncclSend/ncclRecv to rank 0, SC/...RowWise.cpp:85-87); each = (kernel + "
                             "exchange) - kernel alone, max over ranks",
            "host_generation_s": round(t_gen, 1), "plan_create_s": round(t_plan, 2),
            "check": chk,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
    del plan
    comm.close()
    if world > 1:
        dist.destroy_process_group()
    if chk is not None and not chk["ok"]:
        sys.exit(3)


def _x_rows_touched(A, r0: int, r1: int) -> int:
    import numpy as np
    lo, hi = int(A.rowPtr[r0]), int(A.rowPtr[r1])
    return int(np.unique(np.asarray(A.colIndices[lo:hi])).size)


def bench_decomposed(args, world: int, rank: int, local: int, kind: str, K: int, variant: str) -> str | None:
    """N > 1 on a matrix every rank holds (the reference's layout after its
    broadcast, SC/main.cpp:106-143): ONE problem, decomposed like the
    reference's variant (RowWise rows :26-29 / ColumnWise K columns / nnz
    ranges), each rank its share as a distributed plan (tiled where it
    pays), then the one RCCL exchange (all-gather of Y to every rank).  The
    rank-local kernel and the exchange are timed separately too, and the
    independent-copy (replicas) rate is reported beside.  Returns None, or
    the reason when any rank could not build the RCCL communicator (the
    ranks agree over gloo; every rank then returns, and main() runs the
    replicas bench with that reason attached)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import dist as D
    from sparsematrixmultiplicationmpi_amd import inputs

    A, label = build_matrix(kind, args.mtx)
    m, n, nnz = A.numRows, A.numCols, A.nnz
    dl = Deadline(args.phase_timeout, rank, world, metric_for(args.config, K, variant))
    cpu = rank0_cpu_baseline(args, world, rank, dl,
                             lambda: cpu_baseline(A, K, variant, sweep_ranks=False, ranks=cpu_ranks(world)))
    args.cpu_baseline_done = cpu  # (a replicas fallback reports it: the GPU is touched below)
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    # (the other ranks wait for rank 0's CPU baseline in this rendezvous)
    dl.enter("process group + RCCL communicator", seconds=rendezvous_seconds(args, world))
    if world > 1:
        dist.init_process_group("gloo")  # control plane: barrier, max over ranks, RCCL id
    try:
        comm, err = D.Communicator.from_torch_distributed(), None
    except Exception as e:  # e.g. RCCL refusing two ranks on one device (a 1-GPU rehearsal)
        comm, err = None, f"{type(e).__name__}: {e}"
    bad = torch.tensor([0.0 if comm is not None else 1.0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
    if bad.item() > 0:  # (the gloo group stays up for main's replicas bench)
        dl.cancel()
        if comm is not None:
            comm.close()
        return err or "the RCCL communicator failed on another rank"
    rccl_n = comm.nranks()  # the ranks RCCL itself counts (ncclCommCount), reported as n_gpus
    ndevs = _devices_used(dev, world)
    dl.enter("inputs + distributed plans")
    X_host = inputs.generateLargeFatVector(n, K)
    prob_bytes = algorithmic_bytes(m, n, nnz, K)
    ncopies = max(1, min(16, math.ceil(args.cold_bytes / prob_bytes) + 1))
    V = smfv.Variant[variant]
    rows = V in (smfv.Variant.ROWWISE, smfv.Variant.SEQUENTIAL)
    # the plans timed per copy: the value's step first (the default plan: the
    # reference's equal-row blocks, SC/...RowWise.cpp:26-29, all-gathered to
    # every rank), then beside it the reference's exchange semantics (blocks
    # to rank 0 only, MPI_Gatherv / MPI_Reduce, SC/...RowWise.cpp:85-87), the
    # other row partition (SMFV_DIST_BALANCED_ROWS) and the chunked exchange
    # (SMFV_DIST_CHUNKS: chunk j's all-gatherv overlapped with chunk j + 1's
    # compute); a run without --full times the value's step alone
    kinds = {"value": dict(to_all=True, partition=args.partition)}
    if args.full:
        kinds["gather_to_root"] = dict(to_all=False, partition=args.partition)
    if rows and args.full:
        other = "reference" if args.partition == "balanced" else "balanced"
        kinds[f"{other}_rows"] = dict(to_all=True, partition=other)
        if args.chunks > 1:
            kinds[f"chunked{args.chunks}"] = dict(to_all=True, partition=args.partition, chunks=args.chunks)
    copies, t_plan = [], 0.0
    for c in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        dX = torch.from_numpy(X_host).to(dev)
        dY = torch.zeros((m, K), dtype=torch.float64, device=dev)
        t0 = time.time()
        plans = {k: D.DistPlan(comm, V, dA, K, tiles=args.tiles, **kw) for k, kw in kinds.items()}
        torch.cuda.synchronize()
        t_plan += time.time() - t0
        copies.append((plans, dX, dY))
    # at least one untimed step per copy before any capture: RCCL sets up its
    # peer connections on a communicator's first collective, which a graph
    # capture must not contain
    dl.enter("warm-up (first collectives: RCCL connection set-up)")
    for i in range(max(args.warmup, ncopies)):
        plans, dX, dY = copies[i % ncopies]
        for P in plans.values():
            P.run(dX, dY)
    torch.cuda.synchronize()
    dl.enter("timed steps")

    def timed_plan(key, local=False):
        def step(i):
            plans, dX, dY = copies[i % ncopies]
            (plans[key].run_local if local else plans[key].run)(dX, dY)
        return _graph_or_eager(step, args.steps, world)
    ms_step, how = timed_plan("value")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, copies[(args.steps - 1) % ncopies][2])
    ms_loc, how_loc = timed_plan("value", local=True) if args.full else (0.0, None)
    beside = {}
    for key in kinds:
        if key == "value":
            continue
        ms_k, how_k = timed_plan(key)
        ms_kl, _ = timed_plan(key, local=True)
        beside[key] = (ms_k, ms_kl, how_k)
    # correctness after timing: every rank's Y is the whole product (TO_ALL),
    # against the untiled row kernel (pinned to the reference by the tests;
    # not the tiled kernel the ranks' shares run) -- the value's plan and,
    # for ROWWISE, the other TO_ALL plans (--full)
    plans, dX, dY = copies[0]
    ok, ms_rep, reps = True, 0.0, None
    if args.full:
        dl.enter("result check")
        ref_plan = smfv.SpmmPlan(smfv.Variant.SEQUENTIAL, plans["value"].A, K, tiles="off")
        Yseq = torch.empty_like(dY)
        ref_plan.run(dX, Yseq)
        for key, kw in kinds.items():
            if not kw["to_all"]:
                continue
            dY.fill_(float("nan"))
            plans[key].run(dX, dY)
            torch.cuda.synchronize()
            mabs, _ = smfv.compare(Yseq, dY)
            ok &= (mabs == 0.0) if variant != "NONZERO" else (mabs <= 1e-6)
        # secondary: independent copies (every rank its own whole problem)
        reps = [(smfv.SpmmPlan(V, pl["value"].A, K, tiles=args.tiles), dXc, dYc) for pl, dXc, dYc in copies]
        torch.cuda.synchronize()
        ms_rep, _ = _graph_or_eager(lambda i: reps[i % ncopies][0].run(reps[i % ncopies][1], reps[i % ncopies][2]),
                                    args.steps, world)
    first, last, _, _ = plans["value"].partition()
    if rows:
        r0, r1 = int(first[rank]), int(last[rank]) + 1
        loc_bytes = 12 * (int(A.rowPtr[r1]) - int(A.rowPtr[r0])) + 4 * (r1 - r0 + 1) + \
            8 * _x_rows_touched(A, r0, r1) * K + 8 * (r1 - r0) * K
    else:
        loc_bytes = prob_bytes // world
    keys = list(beside)
    # (r6) every rank's local time and bytes: the roofline is the slowest rank's
    per_rank = torch.zeros(2 * world, dtype=torch.float64)
    per_rank[2 * rank], per_rank[2 * rank + 1] = ms_loc, float(loc_bytes)
    if world > 1:
        dist.all_reduce(per_rank)
    vals = [ms_step, ms_loc, ms_rep, float(loc_bytes) / max(ms_loc, 1e-9), 0.0 if ok else 1.0]
    for key in keys:
        vals += [beside[key][0], beside[key][1]]
    t = torch.tensor(vals, dtype=torch.float64)
    tmin = t.clone()
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
    dl.cancel()
    tl = t.tolist()
    ms_step, ms_loc, ms_rep, _, bad = tl[:5]
    flops = 2.0 * nnz * K
    st = plans["value"].stats()
    if rank == 0:
        pr = per_rank.tolist()
        slow = max(range(world), key=lambda r: pr[2 * r])
        s_ms, s_bytes = pr[2 * slow], int(pr[2 * slow + 1])
        # the slowest rank's local bytes / its local time (GB/s)
        loc_gbps = s_bytes / (s_ms * 1e-3) / 1e9 if s_ms > 0 else 0.0
        traffic, traffic_src = measured_rank_traffic(args.config, world, slow, kernel_label(variant, K, st, 8 * n * K))
        others = {}
        for i, key in enumerate(keys):
            ms_k, ms_kl = tl[5 + 2 * i], tl[6 + 2 * i]
            others[key] = {"ms_per_step": round(ms_k, 6), "rank_local_ms": round(ms_kl, 6),
                           "exchange_ms": round(ms_k - ms_kl, 6), "plan": kinds[key],
                           "GFLOPs": round(flops / (ms_k * 1e-3) / 1e9, 3), "timing": beside[key][2]}
        out = {
            "metric": metric_for(args.config, K, variant),
            "value": round(flops / (ms_step * 1e-3) / 1e9, 3),
            "unit": "GFLOP/s", "n_gpus": rccl_n, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 6), "higher_is_better": True, "scaling": "strong",
            "ranks": {"rccl_nranks": rccl_n, "processes": world, "distinct_devices": ndevs},
            "vs_baseline": None, "dtype": "f64",
            "data": f"synthetic: {label}; X = rand()%100+1 (glibc seed 1)",
            "config": {"workload": f"{args.config}: {label} x K={K}, {variant} decomposed over {world} GPUs "
                                   "(rank-local plan + RCCL all-gather of Y)",
                       "m": m, "n": n, "nnz": nnz, "K": K, "variant": variant,
                       "parallelism": f"{variant} partition over {world} ranks "
                                      f"({'work-balanced row blocks' if rows and args.partition == 'balanced' else 'SC partition formulas'}), "
                                      "A and X replicated, Y all-gathered", "copies_rotated": ncopies},
            "roofline": {"bound": "hbm", "achieved": round(loc_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(loc_gbps / HBM_PEAK_GBPS, 4), "traffic": traffic,
                         "traffic_source": traffic_src,
                         "kernel": kernel_label(variant, K, st, 8 * n * K),
                         "rank": slow,
                         "algorithmic_bytes_per_launch": s_bytes,
                         "avg_launch_ms": round(s_ms, 6),
                         "per_rank": [{"rank": r, "local_ms": round(pr[2 * r], 6),
                                       "algorithmic_bytes": int(pr[2 * r + 1])} for r in range(world)],
                         "timing": f"rank-local kernel alone ({how_loc}), slowest rank; traffic: that rank's "
                                   "plan under rocprofv3 PMC on one GPU (bench.py --rank-plans N --rank-only r)"},
            "rank_local_ms": round(ms_loc, 6),
            "exchange_ms": round(ms_step - ms_loc, 6),
            "exchange_ms_gather_to_root": others.get("gather_to_root", {}).get("exchange_ms"),
            "plans_beside": others,
            "exchange_note": "exchange_ms: all-gather of Y to every rank (the value's step); "
                             "plans_beside.gather_to_root: the reference's semantics, blocks gathered to rank 0 "
                             "only (MPI_Gatherv, SC/...RowWise.cpp:85-87 / MPI_Reduce, ...NonZeroElement.cpp:88); "
                             "balanced_rows / reference_rows: the other row partition; chunkedC: C row chunks per "
                             "rank, each chunk's point-to-point all-gatherv started as soon as it is computed; "
                             "each exchange_ms = (kernel + exchange) - kernel alone, max over ranks",
            "timing": how,
            "plan": {"create_s_total": round(t_plan, 3), "tiled": st["tiled"], "reuse": round(st["reuse"], 3),
                     "partition": args.partition if rows else "reference"},
            "check": {"ok": not bad, "criterion": "Y on every rank vs the 1-GPU sequential plan, device compare "
                                                  "(bit-identical; NONZERO 1e-6), every all-gather plan"},
            "replicas": {"note": "every rank its own whole problem, no collective (weak scaling)",
                         "ms_per_step": round(ms_rep, 6),
                         "value_GFLOPs": round(world * flops / (ms_rep * 1e-3) / 1e9, 3) if ms_rep > 0 else None},
            "cpu_baseline": cpu,
            "full": args.full,
        }
        if not args.full:  # (not measured: the value's step alone was timed)
            for k in ("roofline", "rank_local_ms", "exchange_ms", "check", "replicas"):
                out[k] = None
        print(json.dumps(out))
    del copies, reps, plans
    comm.close()
    if world > 1:
        dist.destroy_process_group()
    if bad and not args.no_check:
        sys.exit(3)
    return None


def bench_rank_plans(args, kind: str, K: int, variant: str) -> None:
    """--rank-plans p: a ONE-GPU PROJECTION of the p-GPU decomposition, not a
    scaling measurement.  Every rank r of p runs its share on this one device
    through the product's own rank plan (smfv_dist_plan_create_rank: the same
    partition -- SC/...RowWise.cpp:26-29, ...ColumnWise.cpp:25-28,
    ...NonZeroElement.cpp:24-39 -- and the same single-device plan a rank of
    smfv_dist_plan_create runs), timed alone like the headline (cold rotation
    over copies, one hipGraph of `steps` launches).  Reports the rank-local
    time per rank (max / min), its algorithmic bytes, and the bytes each rank
    contributes to the exchange (RowWise / ColumnWise: its Y block or panel;
    NonZeroElement: its compact partial rows), which the p-GPU step moves over
    xGMI after the slowest rank.  After timing, every rank's share is
    assembled as the exchange would (device copies) and checked against the
    one-GPU untiled sequential plan."""
    import numpy as np
    import torch
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import dist as D
    from sparsematrixmultiplicationmpi_amd import engine as S
    from sparsematrixmultiplicationmpi_amd import inputs

    p = args.rank_plans
    A, label = build_matrix(kind, args.mtx)
    m, n, nnz = A.numRows, A.numCols, A.nnz
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V = smfv.Variant[variant]
    X_host = inputs.generateLargeFatVector(n, K)
    prob_bytes = algorithmic_bytes(m, n, nnz, K)
    ncopies = max(1, min(16, math.ceil(args.cold_bytes / prob_bytes) + 1))
    rowwise = V == smfv.Variant.ROWWISE
    chunks = args.rank_chunks if rowwise else 1
    part = args.partition if rowwise else "reference"
    copies = []
    # (r6) --rank-only r: rank r's plan alone (a PMC run of that rank's kernel)
    sel = [args.rank_only] if 0 <= args.rank_only < p else list(range(p))
    for c in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        dX = torch.from_numpy(X_host).to(dev)
        dY = torch.zeros((m, K), dtype=torch.float64, device=dev)
        plans = [D.DistPlan(None, V, dA, K, to_all=False, rank=(r, p), tiles=args.tiles,
                            tiled_kernel=args.tiled_kernel, partition=part, chunks=chunks) if r in sel else None
                 for r in range(p)]
        copies.append((plans, dX, dY))
    torch.cuda.synchronize()
    first, last, off, cnt = copies[0][0][sel[0]].partition()  # the plans' own partition
    ranks = []
    for r in sel:
        def step(i, r=r):
            plans, dX, dY = copies[i % ncopies]
            plans[r].run_local(dX, dY)
        for i in range(max(args.warmup, ncopies)):
            step(i)
        ms, how = _graph_or_eager(step, args.steps, 1)
        st = copies[0][0][r].stats()
        if V == smfv.Variant.ROWWISE:
            r0, r1 = int(first[r]), int(last[r]) + 1
            lb = 12 * (int(A.rowPtr[r1]) - int(A.rowPtr[r0])) + 4 * (r1 - r0 + 1) + \
                8 * _x_rows_touched(A, r0, r1) * K + 8 * (r1 - r0) * K if r1 > r0 else 0
        elif V == smfv.Variant.COLUMNWISE:
            kc = int(last[r] - first[r] + 1)
            lb = 12 * nnz + 4 * (m + 1) + 8 * n * kc + 8 * m * kc if kc > 0 else 0
        else:
            s_, e_ = _partition_nnz(nnz, p, r)
            rows = int(last[r] - first[r] + 1) if e_ > s_ else 0
            lb = 12 * (e_ - s_) + 8 * _x_rows_touched_nnz(A, s_, e_) * K + 8 * rows * K
        ranks.append({"rank": r, "local_ms": round(ms, 6), "algorithmic_bytes": int(lb),
                      "GBps": round(lb / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                      "exchange_bytes": int(cnt[r]) * 8, "tiled": st["tiled"], "tiles": st["tiles"],
                      "ws_geom": st.get("ws_geom"), "timing": how})
    # the shares assembled as the exchange would, against the 1-GPU sequential plan
    plans, dX, dY = copies[0]
    dY.fill_(float("nan"))
    xbuf = None
    if len(sel) < p:  # one rank: its ROWWISE rows against the same rows of the 1-GPU plan
        ok, mabs = None, None
        if rowwise:
            r = sel[0]
            r0, r1 = int(first[r]), int(last[r]) + 1
            plans[r].run_local(dX, dY)
            ref = smfv.SpmmPlan(smfv.Variant.SEQUENTIAL, plans[r].A, K, tiles="off")
            Yr = torch.empty_like(dY)
            ref.run(dX, Yr)
            mabs, _ = smfv.compare(Yr[r0:r1], dY[r0:r1]) if r1 > r0 else (0.0, None)
            ok = mabs == 0.0
        print(json.dumps({"rank_only": sel[0], "p": p, "config": args.config, "variant": variant,
                          "ranks": ranks, "partition": part,
                          "check": {"ok": ok, "max_abs_diff": mabs,
                                    "criterion": "ROWWISE: the rank's rows vs the 1-GPU untiled sequential plan "
                                                 "(bit-identical); other variants: not assembled with one rank"}}))
        if ok is False and not args.no_check:
            sys.exit(3)
        return
    if V != smfv.Variant.ROWWISE:
        xbuf = torch.full((max(int((off + cnt).max()), 1),), float("nan"), dtype=torch.float64, device=dev)
    for r in range(p):
        plans[r].run_local(dX, dY)
        b = plans[r].exchange_buffer()
        if b is not None and cnt[r] > 0:
            xbuf[int(off[r]):int(off[r] + cnt[r])] = b[int(off[r]):int(off[r] + cnt[r])]
    if V == smfv.Variant.COLUMNWISE:
        smfv._lib.call("smfv_panels_to_rowmajor_f64", m, K, p, xbuf.data_ptr(), dY.data_ptr(), K, S.stream_handle())
    elif V == smfv.Variant.NONZERO:
        import ctypes
        rfa = (ctypes.c_int * p)(*[int(v) for v in first])
        rla = (ctypes.c_int * p)(*[int(v) for v in last])
        smfv._lib.call("smfv_combine_row_blocks_f64", m, K, p, rfa, rla, xbuf.data_ptr(), dY.data_ptr(), K,
                       S.stream_handle())
    ref = smfv.SpmmPlan(smfv.Variant.SEQUENTIAL, plans[0].A, K, tiles="off")
    Yr = torch.empty_like(dY)
    ref.run(dX, Yr)
    mabs, _ = smfv.compare(Yr, dY)
    ok = mabs == 0.0 if V != smfv.Variant.NONZERO else mabs <= 1e-6
    loc = [x["local_ms"] for x in ranks]
    flops = 2.0 * nnz * K
    xbytes = [x["exchange_bytes"] for x in ranks]
    # (r5) the exchange the p-GPU step adds, projected (not measured: no
    # multi-GPU box): TO_ALL over xGMI's full mesh with point-to-point sends,
    # every GPU sends its block to each of the p - 1 peers on its own link and
    # receives theirs, so each link carries one block per direction and the
    # exchange takes ~ the largest block / the link rate.  The rate is
    # SURVEY 5's ~153 GB/s per link (--xgmi-gbps), read as per direction;
    # `half_rate_us` reads it as both directions together.  Chunked (C row
    # chunks, chunk j's exchange while chunk j + 1 computes): with equal
    # chunks, max(L / C + E, L + E / C) for rank-local time L and exchange E
    # (chunk compute taken as L / C: a lower bound, a chunk's plan has its
    # own fill and drain).
    link = args.xgmi_gbps * 1e9
    E_us = max(xbytes) / link * 1e6 if p > 1 else 0.0
    L_us = max(loc) * 1e3
    proj = {"assumption": f"xGMI full mesh, {args.xgmi_gbps:.0f} GB/s per link per direction (SURVEY 5, "
                          "unmeasured here); TO_ALL as point-to-point sends, one block per link per direction",
            "links_used_per_gpu": p - 1, "bytes_per_link_per_direction_max": max(xbytes) if p > 1 else 0,
            "bytes_received_per_gpu_max": int(sum(xbytes) - min(xbytes)) if p > 1 else 0,
            "exchange_us": round(E_us, 3), "exchange_us_half_rate": round(2 * E_us, 3),
            "rank_local_us_max": round(L_us, 3),
            "step_us": round(L_us + E_us, 3), "step_us_half_rate": round(L_us + 2 * E_us, 3),
            "GFLOPs": round(flops / ((L_us + E_us) * 1e-6) / 1e9, 1) if L_us + E_us > 0 else None}
    if rowwise and p > 1:
        for C in (2, 4):
            proj[f"step_us_chunked{C}"] = round(max(L_us / C + E_us, L_us + E_us / C), 3)
    print(json.dumps({
        "projection": f"{p}-GPU decomposition projected on ONE GPU (each rank's share timed alone, in turn); "
                      "not a scaling measurement: no RCCL, no concurrent ranks",
        "metric": metric_for(args.config, K, variant), "unit": "us", "config": args.config, "variant": variant,
        "p": p, "steps": args.steps, "copies_rotated": ncopies,
        "rank_local_us_max": round(max(loc) * 1e3, 3), "rank_local_us_min": round(min(loc) * 1e3, 3),
        "ideal_us_1_over_p_of_1gpu": None,
        "projected_GFLOPs_without_exchange": round(flops / (max(loc) * 1e-3) / 1e9, 1),
        "exchange_bytes_max": max(xbytes), "exchange_bytes_total": int(sum(xbytes)),
        "exchange_note": "bytes a rank's block adds to the exchange (TO_ALL: every rank receives all others' "
                         "blocks: the all-gather moves (p-1)/p of the total into each GPU)",
        "exchange_projection": proj,
        "partition": part, "rank_chunks": chunks,
        "ranks": ranks, "tiled_kernel": args.tiled_kernel,
        "check": {"ok": bool(ok), "max_abs_diff": mabs,
                  "criterion": "shares assembled as the exchange would vs the 1-GPU untiled sequential plan "
                               "(bit-identical; NONZERO 1e-6)"}}))
    if not ok and not args.no_check:
        sys.exit(3)


def _partition_nnz(nnz: int, p: int, r: int):
    """Rank r's nnz range [s, e) of SC/...NonZeroElement.cpp:24-39 (smfv_partition_nnz)."""
    q, extra = divmod(nnz, p)
    s = r * (q + 1) if r < extra else r * q + extra
    return s, s + q + (1 if r < extra else 0)


def _x_rows_touched_nnz(A, s: int, e: int) -> int:
    import numpy as np
    return int(np.unique(np.asarray(A.colIndices[s:e])).size) if e > s else 0


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(n: int, argv: list[str]) -> int:
    """`bench.py --gpus N` (N > 1) without WORLD_SIZE: start the N ranks as
    fresh child processes -- torch.distributed.run on 127.0.0.1, one rank per
    GPU, this same script and arguments -- before anything touches the GPU
    (no exec: the parent only waits), then re-print rank 0's JSON line as
    this process's one stdout line.  Everything else the ranks write goes to
    stderr.  The exit status is the ranks' (torch.distributed.run's).  The
    line's n_gpus is what the ranks measured (the RCCL communicator's own
    count in decomposed mode), and a line whose n_gpus is not N makes the
    exit status non-zero."""
    import signal
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + argv
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    print(f"[bench] --gpus {n} without WORLD_SIZE: starting {n} ranks: {' '.join(cmd[1:])}", file=sys.stderr,
          flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)

    def forward(sig, _frame):  # a timeout / kill of the parent ends the ranks too
        proc.send_signal(sig)
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, forward)
    lines = []
    for line in proc.stdout:
        if line.lstrip().startswith("{"):
            lines.append(line.strip())
        sys.stderr.write(line)
        sys.stderr.flush()
    rc = proc.wait()
    out = None
    for line in reversed(lines):
        try:
            obj = json.loads(line)
        except ValueError:
            continue
        if "metric" in obj or "dry_run" in obj:
            out = obj
            break
    if out is None:
        print(json.dumps({"metric": HEADLINE_METRIC, "value": None, "unit": "GFLOP/s", "n_gpus": n,
                          "error": f"the {n} ranks printed no result line (exit status {rc})"}), flush=True)
        return rc or 5
    out["launcher"] = {"ranks_started": n, "how": "bench.py --gpus N without WORLD_SIZE: N child ranks via "
                                                  "torch.distributed.run --nproc-per-node N (127.0.0.1)"}
    print(json.dumps(out), flush=True)
    if rc == 0 and out.get("n_gpus") != n:
        print(f"[bench] the ranks reported n_gpus {out.get('n_gpus')}, not {n}", file=sys.stderr)
        return 6
    return rc


def dry_run(args, world: int, rank: int, local: int) -> None:
    """--dry-run: the ranks start and meet (gloo), nothing touches the GPU;
    rank 0 prints who came (tests the launcher on a CPU host) and (r6) the
    CPU baseline the N-GPU line would carry, timed the same way (rank 0 first,
    the others waiting in the rendezvous)."""
    import torch.distributed as dist
    me = {"rank": rank, "local_rank": local, "pid": os.getpid()}
    ranks = [me]
    kind, K, variant = CONFIGS[args.config]
    variant = args.variant or variant
    cpu = None
    if kind in ("cop20k", "cop20k_perm", "cop20k_irr"):
        dl = Deadline(args.phase_timeout, rank, world, metric_for(args.config, K, variant))
        cpu = rank0_cpu_baseline(args, world, rank, dl, lambda: cpu_baseline(
            build_matrix(kind, args.mtx)[0], K, variant, sweep_ranks=False, ranks=cpu_ranks(world)))
        dl.cancel()
    if world > 1:
        dist.init_process_group("gloo")
        ranks = [None] * world
        dist.all_gather_object(ranks, me)
        seen = dist.get_world_size()
        dist.destroy_process_group()
    else:
        seen = 1
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": seen, "ranks": ranks, "cpu_baseline": cpu}), flush=True)


def _devices_used(dev, world: int) -> int:
    """Distinct GPUs (PCI domain:bus:device) the ranks run on, over gloo."""
    import torch
    import torch.distributed as dist
    pr = torch.cuda.get_device_properties(dev)
    key = f"{getattr(pr, 'pci_domain_id', 0)}:{getattr(pr, 'pci_bus_id', dev.index)}:" \
          f"{getattr(pr, 'pci_device_id', 0)}"
    if world == 1:
        return 1
    keys = [None] * world
    dist.all_gather_object(keys, key)
    return len(set(keys))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one per GPU); > 1 without WORLD_SIZE starts them itself (torch.distributed.run); "
                         "under torch.distributed.run it must equal WORLD_SIZE")
    ap.add_argument("--dry-run", action="store_true",
                    help="start the ranks and have them meet (gloo) without touching the GPU; rank 0 prints them")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="cop20k_k32", choices=sorted(CONFIGS))
    ap.add_argument("--mtx", default=os.environ.get("SMFV_COP20K_MTX"))
    ap.add_argument("--variant", default=None, choices=["SEQUENTIAL", "ROWWISE", "COLUMNWISE", "NONZERO"])
    ap.add_argument("--mode", default=None, choices=["decomposed", "replicas"],
                    help="one problem decomposed over the ranks (default for N > 1; at N = 1 it runs the "
                         "distributed plan with one rank) or one copy per rank (default for N = 1)")
    ap.add_argument("--cold-bytes", type=float, default=1.0e9,
                    help="rotate copies until this many bytes separate two uses of one copy")
    ap.add_argument("--tiles", default="auto", choices=["auto", "off", "force"],
                    help="row-tile LDS staging of the plan (SpmmPlan tiles=)")
    ap.add_argument("--split-ends", action="store_true",
                    help="half tiles first and last in every block (SMFV_PLAN_SPLIT_ENDS, A/B; measured slower)")
    ap.add_argument("--seeds", default="frontier", choices=["frontier", "natural"],
                    help="tile seeding of the plan (SMFV_PLAN_NATURAL_SEEDS for natural)")
    ap.add_argument("--xcd-parts", default="auto", choices=["auto", "one"],
                    help="XCD tile ranges of the plan: row range per XCD when the footprint allows (auto) "
                         "or one wavefront cut in 8 (one: SMFV_PLAN_ONE_WAVEFRONT, A/B)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--rows", type=int, default=0, help="syn80m_k32: matrix rows (default 80M)")
    ap.add_argument("--no-vendor", action="store_true", help="skip the rocSPARSE comparator leg")
    ap.add_argument("--no-warm", action="store_true",
                    help="skip the same-copy (warm) leg: every launch of the process streams from HBM "
                         "(for a cold-only rocprofv3 kernel trace)")
    ap.add_argument("--no-copy-floor", action="store_true",
                    help="skip the size-matched copy (roofline.size_matched_copy)")
    ap.add_argument("--no-rebind", action="store_true",
                    help="skip the bind + execute leg (values changed every step; plan.rebind_each_step)")
    ap.add_argument("--no-check", action="store_true",
                    help="report the post-timing result check but do not fail on it (lab ablations)")
    ap.add_argument("--mfma", action="store_true",
                    help="time the opt-in dense-block MFMA tile kernel (SMFV_PLAN_MFMA, config 3's MFMA K-panel)")
    ap.add_argument("--tiled-kernel", default="auto", choices=["auto", "ws", "ws1", "ws2", "ws3"],
                    help="tiled kernel for K % 32 == 0: the library's choice or k_rows_ws (SMFV_PLAN_WS), A/B; "
                         "ws1 / ws2 / ws3: k_rows_ws with one 1024-lane / two 512-lane / one 768-lane pipeline(s) "
                         "per CU (SMFV_PLAN_WS_GEOM1 / 2 / 3)")
    ap.add_argument("--live-values", action="store_true",
                    help="tiled plans read the live CSR values (SMFV_PLAN_LIVE_VALUES: no snapshot, bind a no-op)")
    ap.add_argument("--row-pairs", default="auto", choices=["auto", "on", "off"],
                    help="row pairs in k_rows_ws tiles: the plan with fewer rounds (auto), forced on / off (A/B)")
    ap.add_argument("--fma", action="store_true",
                    help="time the opt-in FMA plans (SMFV_PLAN_FMA) instead of the bit-exact ones")
    ap.add_argument("--rank-plans", type=int, default=0,
                    help="p > 0: a one-GPU projection of the p-rank decomposition -- every rank's share timed in "
                         "turn through its rank plan (smfv_dist_plan_create_rank); prints a projection line, not "
                         "the headline")
    ap.add_argument("--partition", default="reference", choices=["balanced", "reference"],
                    help="decomposed / --rank-plans ROWWISE: the reference's equal row counts (SC/...RowWise.cpp:26-29, "
                         "default) or row blocks of equal work (SMFV_DIST_BALANCED_ROWS)")
    ap.add_argument("--chunks", type=int, default=1,
                    help="decomposed ROWWISE: also time the chunked exchange with this many row chunks per rank "
                         "(SMFV_DIST_CHUNKS; 1 = skip, the default: its point-to-point RCCL groups have not run on "
                         "more than one GPU yet, so the driver's run does not depend on them)")
    ap.add_argument("--rank-only", type=int, default=-1,
                    help="--rank-plans: time only this rank's plan (a PMC run of one rank's kernel); its share is "
                         "checked against the 1-GPU sequential plan's rows")
    ap.add_argument("--rank-chunks", type=int, default=1,
                    help="--rank-plans ROWWISE: row chunks per rank plan (SMFV_DIST_CHUNKS; each chunk its own plan)")
    ap.add_argument("--xgmi-gbps", type=float, default=153.0,
                    help="--rank-plans: xGMI GB/s per link per direction assumed by the exchange projection "
                         "(SURVEY 5: 7 links of ~153 GB/s per GPU; not measured on this pool)")
    ap.add_argument("--phase-timeout", type=float, default=240.0,
                    help="multi-GPU paths: seconds a phase (RCCL set-up, plans, warm-up, timing, check) may take "
                         "before a diagnostic JSON line and exit status 4 (0 = no watchdog)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: the CPU baseline, nine more timed regions (their "
                         "median, min and max), the bind / rebind, warm, copy-floor and rocSPARSE legs, the plans "
                         "timed beside a decomposed step, and the post-timing result check.  Without it a run sets "
                         "up, warms up, times --steps steps and prints the result line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (Y, on rank 0) as "
                         "DIR/Y.npy in float64; an output over 64 MB is written as a fixed sample of its rows")
    args = ap.parse_args()
    if args.dump_outputs and args.rank_plans > 0:
        ap.error("--dump-outputs: a --rank-plans projection has no one output (every rank's share is timed in turn)")
    if not args.full:  # a plain run measures the headline figure only
        args.no_cpu_baseline = args.no_vendor = args.no_warm = args.no_copy_floor = args.no_rebind = True

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and (args.gpus or 1) > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(env_world or "1")
    if args.gpus is not None and args.gpus != world:
        print(json.dumps({"metric": HEADLINE_METRIC, "value": None, "unit": "GFLOP/s", "n_gpus": world,
                          "error": f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher started a different "
                                   "number of ranks than asked"}), flush=True)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        dry_run(args, world, rank, local)
        return
    kind, K, variant = CONFIGS[args.config]
    variant = args.variant or variant
    if kind == "syn80m":
        bench_rowpart(args, world, rank, local, K)
        return
    if args.rank_plans > 0:
        bench_rank_plans(args, kind, K, variant)
        return
    mode = args.mode or ("decomposed" if world > 1 else "replicas")
    fallback = None
    if mode == "decomposed" and kind in ("cop20k", "cop20k_perm", "cop20k_irr"):
        fallback = bench_decomposed(args, world, rank, local, kind, K, variant)
        if fallback is None:
            return
        print(f"[bench] decomposed mode unavailable ({fallback}); timing replicas instead", file=sys.stderr)

    A, label = build_matrix(kind, args.mtx)
    m, n, nnz = A.numRows, A.numCols, A.nnz
    cop = kind in ("cop20k", "cop20k_perm", "cop20k_irr")

    # CPU baseline first: rank 0 at N = 1, before anything touches the GPU
    # (r6: at every N; rank 0, the other ranks wait in the gloo rendezvous)
    cpu = None
    if rank == 0 and not args.no_cpu_baseline:
        if fallback is not None:
            cpu = getattr(args, "cpu_baseline_done", None)  # timed by bench_decomposed before the GPU
        elif cop:
            cpu = cpu_baseline(A, K, variant, ranks=cpu_ranks(world))
        else:  # bounded stand-in: a 1M x 1M instance of the same generator (same row-length law)
            from sparsematrixmultiplicationmpi_amd import inputs
            S = inputs.gen_random_rows(1_000_000, 1_000_000, 16.0, 2.0, 4096, 42)
            cpu = cpu_baseline(S, K, variant, sample="bounded sample: 1M x 1M instance of the same power-law "
                                                     f"generator (nnz {S.nnz}), K={K}", sweep_ranks=False,
                               ranks=cpu_ranks(world))

    import torch
    import torch.distributed as dist
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import inputs, sampling

    # one process per GPU; (local % devices) also lets a 1-GPU box rehearse N > 1
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    if world > 1 and not dist.is_initialized():
        # --mode replicas: control plane only (barrier + max over ranks), every
        # rank runs its own copy of the problem (a decomposed-mode fallback
        # arrives with the group already up)
        dist.init_process_group("gloo")
    procs = dist.get_world_size() if world > 1 else 1  # the ranks that actually joined
    ndevs = _devices_used(dev, world)

    # ---- resident problem copies ----------------------------------------
    X_host = inputs.generateLargeFatVector(n, K) if cop else None
    prob_bytes = algorithmic_bytes(m, n, nnz, K)
    ncopies = max(1, min(16, math.ceil(args.cold_bytes / prob_bytes) + 1))
    copies, t_plan = [], []
    for c in range(ncopies):
        dA = smfv.DeviceCSR(A, dev)
        if X_host is not None:
            dX = torch.from_numpy(X_host).to(dev)
        else:
            dX = torch.empty((n, K), dtype=torch.float64, device=dev)
            smfv.fill_x_hash(dX, 43)
        dY = torch.empty((m, K), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.time()
        plan = smfv.SpmmPlan(smfv.Variant[variant], dA, K, tiles=args.tiles, fma=args.fma, seeds=args.seeds,
                             mfma=args.mfma, split_ends=args.split_ends, xcd_parts=args.xcd_parts,
                             tiled_kernel=args.tiled_kernel, live_values=args.live_values,
                             row_pairs=args.row_pairs)
        torch.cuda.synchronize()
        t_plan.append(time.time() - t0)
        copies.append((plan, dX, dY))
    torch.cuda.synchronize()
    # bind cost (the values snapshot gather of a tiled plan), timed on its own (--full)
    bind_ms = _timed_events(lambda: [copies[0][0].bind_values() for _ in range(20)], 1) / 20 if args.full else None

    def step(i: int, warm: bool = False):
        plan, dX, dY = copies[0 if warm else i % ncopies]
        plan.run(dX, dY)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()

    # The timed steps are captured into one hipGraph (torch.cuda.CUDAGraph on a
    # side stream): a ~40 us launch issued from Python + ctypes one by one is
    # host-bound, the graph replay is not.  Inputs stay resident; nothing is
    # skipped: the graph holds exactly `steps` SpMM launches.
    def capture(warm: bool, count: int = args.steps):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(count):
                    step(i, warm)
        torch.cuda.current_stream().wait_stream(side)
        return g

    def timed(g):
        return _timed_events(g.replay, world)

    stabilize_replays = []

    st0 = copies[0][0].stats()
    # more steps than GRAPH_CHUNK: one graph of whole rotations over the
    # copies, replayed back to back, and one of the remaining steps, so the
    # timed region still holds exactly `steps` launches in rotation order
    chunk = max(1, GRAPH_CHUNK // ncopies) * ncopies
    whole, rest = divmod(args.steps, chunk) if args.steps > chunk else (0, args.steps)
    side = min(args.steps, chunk)  # launches per graph of the legs timed beside the value (--full)
    g_chunk = capture(False, chunk) if whole else None
    g_rest = capture(False, rest) if rest else None
    stabilize_replays.append(_stabilize(g_chunk or g_rest))

    def replay_cold():
        for _ in range(whole):
            g_chunk.replay()
        if g_rest is not None:
            g_rest.replay()

    first_ms = _timed_events(replay_cold, world)
    if args.dump_outputs and rank == 0:  # the last timed step's Y, before any other leg writes it
        dump_outputs(args.dump_outputs, copies[(args.steps - 1) % ncopies][2])
    # --full: nine more samples of the same K steps: `value` is then the median
    # of the ten timed regions (hipEvents around >= 200 launches per
    # sample, median of 10 samples; the upper median for an even count); the
    # first region, min and max are reported beside it.  A plain run's value
    # is its one timed region.
    samples = sorted([first_ms] + [_timed_events(replay_cold, world) for _ in range(9 if args.full else 0)])
    span_ms = samples[len(samples) // 2]
    del g_chunk, g_rest
    # bind + execute per step with the values changed every step (an
    # iterative caller whose matrix values change between products): each
    # copy alternates between two value arrays, every step re-binds its plan
    # (the values snapshot) and runs it, all in one graph; the bind alone
    # the same way.  Reported in `plan`, not in `value`.
    rebind = None
    if not args.no_rebind:
        from sparsematrixmultiplicationmpi_amd._lib import call as _call
        alt = [(plan.A.values, plan.A.values * 0.5 + 1.0) for plan, _, _ in copies]
        torch.cuda.synchronize()

        def rb_step(i, execute=True, plans=None):
            plan, dX, dY = copies[i % ncopies]
            plan = plan if plans is None else plans[i % ncopies]
            vals = alt[i % ncopies][(i // ncopies) % 2]
            st_ = torch.cuda.current_stream().cuda_stream
            _call("smfv_plan_bind_values", plan._plan, vals.data_ptr(), st_)
            if execute:
                rp_, ci_, _ = plan.A.ptrs()
                _call("smfv_plan_execute", plan._plan, rp_, ci_, vals.data_ptr(), dX.data_ptr(), K, dY.data_ptr(), K,
                      st_)
        ms_be, how_be = _graph_or_eager(lambda i: rb_step(i, True), side, world)
        ms_b, _ = _graph_or_eager(lambda i: rb_step(i, False), side, world)
        for plan, _, _ in copies:  # back to the values the check uses
            plan.bind_values()
        torch.cuda.synchronize()
        rebind = {"bind_plus_execute_ms": round(ms_be, 6), "bind_ms": round(ms_b, 6),
                  "bind_descriptors": st0.get("bind_descriptors"),
                  "GFLOPs_incl_bind": round(2.0 * nnz * K / (ms_be * 1e-3) / 1e9, 3),
                  "frac_incl_bind": round(prob_bytes / (ms_be * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                  "timing": how_be,
                  "note": "every step binds its plan to values that changed since its last bind (two arrays "
                          "alternating per copy) and executes; bind_ms: the binds alone, same rotation"}
        # (r5) the same with live-values plans (SMFV_PLAN_LIVE_VALUES: the
        # tiled kernel reads the CSR values itself, a bind is a no-op) -- the
        # plan a caller whose values change every product would take
        if st0.get("kernel") == "k_rows_ws" and not st0.get("live_values"):
            live = [smfv.SpmmPlan(smfv.Variant[variant], pl.A, K, tiles=args.tiles, fma=args.fma, seeds=args.seeds,
                                  split_ends=args.split_ends, xcd_parts=args.xcd_parts,
                                  tiled_kernel=args.tiled_kernel, live_values=True) for pl, _, _ in copies]
            torch.cuda.synchronize()
            if all(lp.stats()["live_values"] for lp in live):
                ms_lbe, how_l = _graph_or_eager(lambda i: rb_step(i, True, live), side, world)
                rebind["live_values"] = {
                    "bind_plus_execute_ms": round(ms_lbe, 6),
                    "GFLOPs_incl_bind": round(2.0 * nnz * K / (ms_lbe * 1e-3) / 1e9, 3),
                    "frac_incl_bind": round(prob_bytes / (ms_lbe * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                    "timing": how_l,
                    "note": "live-values plans (SMFV_PLAN_LIVE_VALUES) of the same copies, same value changes: "
                            "the bind is a no-op, the kernel DMAs each value pair from the CSR values"}
                best = min(ms_be, ms_lbe)
                rebind["best_bind_plus_execute_ms"] = round(best, 6)
                rebind["best_plan"] = "live_values" if ms_lbe < ms_be else "snapshot"
            del live
            torch.cuda.synchronize()
    # the warm leg (same copy every launch) after the cold one; --no-warm
    # leaves it out so a profile of this process holds cold launches only
    span_ms_w = float("nan")
    if not args.no_warm:
        g_warm = capture(True, side)
        stabilize_replays.append(_stabilize(g_warm))
        span_ms_w = timed(g_warm)
        del g_warm
    stream_gbps = stream_copy_gbps(dev) if args.full else None
    copy_floor = size_matched_copy(dev, prob_bytes, ncopies, side, world) if not args.no_copy_floor else None
    wr_bytes = 8 * m * K
    mix_floor = (mix_matched_copy(dev, prob_bytes - wr_bytes, wr_bytes, ncopies, side, world)
                 if not args.no_copy_floor else None)
    vendor = None
    if variant in ("ROWWISE", "SEQUENTIAL") and not args.no_vendor:
        vendor = vendor_leg(copies, side, timed, 2.0 * nnz * K)
    ms_per_step = span_ms / args.steps
    kern_ms = ms_per_step  # average launch duration incl. the graph's kernel boundaries
    kern_ms_w = span_ms_w / side
    if world > 1:
        t = torch.tensor([ms_per_step, kern_ms, kern_ms_w], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms_per_step, kern_ms, kern_ms_w = t.tolist()
        span_ms_w = kern_ms_w * side

    # result check after timing: configs 4 (sampled rows; the full reference
    # result is too large for the host) and the cop20k configs (device compare
    # against the untiled row kernel, bit for bit); --full
    chk = None
    plan, dX, dY = copies[0]
    if args.full:
        plan.run(dX, dY)
        torch.cuda.synchronize()
    if args.full and rank == 0 and not cop:
        rows = sampling.sample_rows(A.rowPtr, K)
        chk = sampled_check(A, rows, dX, dY, exact=variant != "NONZERO")
    elif args.full and rank == 0:
        ref = smfv.SpmmPlan(smfv.Variant.SEQUENTIAL, plan.A, K, tiles="off")
        Yr = torch.empty_like(dY)
        ref.run(dX, Yr)
        mabs, _ = smfv.compare(Yr, dY)
        ok = mabs == 0.0 if not (variant == "NONZERO" or args.fma or args.mfma) else mabs <= 1e-6
        chk = {"ok": bool(ok), "max_abs_diff": mabs,
               "criterion": "vs the untiled row kernel (pinned bit-identical to the reference by the tests)"}

    flops = 2.0 * nnz * K
    st = copies[0][0].stats()
    kname = kernel_label(variant, K, st, 8 * n * K)
    traffic, traffic_src = measured_traffic(args.config, kname) if args.tiles != "force" else (None, None)
    value = world * flops / (ms_per_step * 1e-3) / 1e9
    achieved = prob_bytes / (kern_ms * 1e-3) / 1e9
    achieved_w = prob_bytes / (kern_ms_w * 1e-3) / 1e9
    if rank == 0:
        out = {
            "metric": metric_for(args.config, K, variant),
            "value": round(value, 3),
            "unit": "GFLOP/s",
            "n_gpus": procs,
            "ranks": {"processes": procs, "distinct_devices": ndevs,
                      "note": "replicas: one independent problem per rank, no RCCL"},
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 6),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": f"synthetic: {label}; X = rand()%100+1 (glibc seed 1)" if cop else f"synthetic: {label}",
            "config": {"workload": f"{args.config}: {label} x K={K}, {variant} HIP kernel",
                       "m": m, "n": n, "nnz": nnz, "K": K, "variant": variant,
                       "parallelism": f"{world} GPU(s), one independent problem copy per GPU",
                       "copies_rotated": ncopies},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                         "traffic_source": traffic_src,
                         "kernel": kname,
                         "algorithmic_bytes_per_launch": prob_bytes,
                         "avg_launch_ms": round(kern_ms, 6),
                         "timing": "HIP events around the hipGraph replay of all timed launches (one graph up to "
                                   f"{GRAPH_CHUNK} launches, else that graph replayed back to back); "
                                   + ("median of 10 such timed regions" if args.full else "one timed region"),
                         "untimed_replays_before_timing": stabilize_replays,
                         "samples_ms_per_step": {"n": len(samples), "median": round(samples[len(samples) // 2] / args.steps, 6),
                                                 "first_region": round(first_ms / args.steps, 6),
                                                 "min": round(samples[0] / args.steps, 6),
                                                 "max": round(samples[-1] / args.steps, 6)},
                         "stream_copy_GBps": round(stream_gbps, 1) if stream_gbps else None,
                         "frac_of_stream_copy": round(achieved / stream_gbps, 4) if stream_gbps else None,
                         "size_matched_copy": (dict(copy_floor, frac_of_copy_time=round(copy_floor["avg_launch_ms"] / kern_ms, 4))
                                               if copy_floor else None),
                         "mix_matched_copy": (dict(mix_floor, **{f"frac_of_spmm_time_{k}": round(
                             mix_floor[k]["avg_launch_ms"] / kern_ms, 4) for k in ("plain", "lds32", "lds64")})
                                              if mix_floor else None),
                         "lds_staged_bytes_per_launch": lds_staged_bytes(st, K)},
            "plan": {"tiled": st["tiled"], "tiles": st["tiles"], "reuse": round(st["reuse"], 3),
                     "live_values": st["live_values"], "paired_rows": st.get("paired_rows"),
                     "est_reuse_sampled": round(st["est_reuse"], 3), "direct_rows": st["direct_rows"],
                     "create_s": round(t_plan[0], 3), "analysis_ms": round(st["analysis_ms"], 1),
                     "bind_ms": round(bind_ms, 4) if bind_ms is not None else None, "snapshot_entries": st["snapshot_entries"],
                     "rebind_each_step": rebind,
                     "xcd_parts": st["xcd_parts"], "footprint_8_ranges": round(st["footprint"], 3),
                     "note": "create = host analysis + upload, once per pattern; bind = values snapshot "
                             "gather, once per value change; neither is in the timed step"},
            "gather_model": ({"bytes_per_launch": prob_bytes + 8 * nnz * K,
                              "GBps": round((prob_bytes + 8 * nnz * K) / (kern_ms * 1e-3) / 1e9, 1),
                              "note": "random columns: one X row gathered per non-zero (SURVEY 8d config 4)"}
                             if kind == "pow10m" else None),
            "warm": ({"note": "same copy every launch (working set in the 256 MiB Infinity Cache)",
                      "avg_launch_ms": round(kern_ms_w, 6), "achieved_GBps": round(achieved_w, 1),
                      "GFLOPs": round(world * flops / (span_ms_w / side * 1e-3) / 1e9, 3)}
                     if not args.no_warm else None),
            "effective_GFLOPs_per_gpu": round(flops / (ms_per_step * 1e-3) / 1e9, 3),
            "check": chk,
            "cpu_baseline": cpu,
            "vendor_rocsparse": vendor,
            "full": args.full,
        }
        if args.dump_outputs:
            out["dumped_outputs"] = os.path.join(args.dump_outputs, "Y.npy")
        if fallback is not None:
            out["decomposed_fallback"] = {"reason": fallback,
                                          "note": "the decomposed (RCCL) mode could not start; these are replicas"}
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()
    if chk is not None and not chk["ok"] and not args.no_check:
        sys.exit(3)


if __name__ == "__main__":
    main()
