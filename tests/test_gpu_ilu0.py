"""ILU(0) on the GPU (smfv_ilu0_plan_*, Ilu0Plan, ilu0, Ilu0Preconditioner):
every result is compared bit for bit (adversarial.same: NaN for NaN, the sign
of zero included) with the loop of include/smfv.h restated in numpy
(tests/ilu0_ref.py, never the library).

Inputs, m <= 3000: `band` (953 levels, nearly all a few rows thin), `grid9`
(wider levels), `long_row` (an arrow: one row of 3,000 entries and 2,999 steps
at the end of a 3000-level chain), `wide` (8 levels of 375 rows, every step
full of pairs), the degenerate shapes and the special-values case, whose
reference is at least 80 % finite (asserted where it is built).  The three
chain settings -- auto, one launch per level, everything in the one-block
kernel -- must give the same bits, and stats() must show the path each case
is for.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
import ilu0_ref as R
import trsm_ref as T
from test_gpu_capture import NAN, capture, in_stream_order

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd._lib import SmfvError, call, lib
from sparsematrixmultiplicationmpi_amd.engine import stream_handle

pytestmark = pytest.mark.gpu
IP = ctypes.POINTER(ctypes.c_int)
CHAINS = ("auto", "off", "all")
GUARD = 64  # NaN doubles on each side of F


def csr_of(A, gpu):
    return smfv.DeviceCSR(smfv.SparseMatrix(np.array(A.values), np.array(A.colIndices), np.array(A.rowPtr), A.numRows,
                                            A.numCols), gpu)


@functools.lru_cache(maxsize=None)
def shared_csr(name, gpu):
    """The DeviceCSR of a named input, shared and read-only."""
    return csr_of(R.reference(name)[0], gpu)


def guarded(nnz, gpu):
    """A NaN-filled buffer and the nnz doubles of F inside it."""
    buf = torch.full((nnz + 2 * GUARD,), NAN, dtype=torch.float64, device=gpu)
    return buf, buf[GUARD:GUARD + nnz]


def read(buf, nnz):
    """F on the host; the guard elements must still be NaN."""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + nnz:]).all(), "F written outside its range"
    return np.ascontiguousarray(h[GUARD:GUARD + nnz])


def three_ways(name, gpu):
    """auto / off / all against the loop (hence against each other), into a
    separate guarded buffer with the input unchanged; returns the stats."""
    A, f = R.reference(name)
    dA = shared_csr(name, gpu)
    stats = {}
    for chain in CHAINS:
        plan = smfv.Ilu0Plan(dA, chain)
        buf, F = guarded(dA.nnz, gpu)
        assert plan.factor(F) is F
        assert adv.same(read(buf, dA.nnz), f), (name, chain)
        assert adv.same(dA.values.cpu().numpy(), np.asarray(A.values)), "the input changed"
        stats[chain] = plan.stats()
    a, o, c = (stats[k] for k in CHAINS)
    print("ILU0", name, {k: (v["launches"], v["chain_launches"]) for k, v in stats.items()})
    assert o["launches"] == o["levels"] == a["levels"] and o["chain_launches"] == 0
    assert c["launches"] == c["chain_launches"] == (1 if dA.m else 0) and c["chain_rows"] == dA.m
    assert c["chain_max_levels"] == c["levels"]
    cnt = R.counts_of(name)
    for st in stats.values():
        assert (st["steps"], st["pairs"], st["long_rows"]) == (cnt["steps"], cnt["pairs"], cnt["long_rows"])
        assert st["plan_bytes"] > 0 and st["lds_slot_entries"] == R.SLOT
    return stats


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
def test_band(gpu):
    a = three_ways("band", gpu)["auto"]
    assert a["levels"] == 953 and a["long_rows"] == 0
    assert a["chain_launches"] > 0 and a["chain_max_levels"] > 100 and a["launches"] < a["levels"] // 10


def test_grid9(gpu):
    st = three_ways("grid9", gpu)
    assert st["auto"]["levels"] == 70 and st["off"]["launches"] == 70


def test_long_row(gpu):
    """A row of 3,000 entries and 2,999 steps: a whole block eliminates it in F
    itself, in the grid kernel (off) and in the one-block kernel (auto, all)."""
    st = three_ways("long_row", gpu)
    for s in st.values():
        assert s["long_rows"] == 1 and s["max_steps_per_row"] == 2999 > s["lds_slot_entries"]
    assert st["auto"]["levels"] == 3000 == st["off"]["launches"] and st["auto"]["chain_max_levels"] == 3000


def test_wide(gpu):
    st = three_ways("wide", gpu)
    a = st["auto"]
    assert a["levels"] == 8 == a["launches"] and a["widest_level"] == 375 and a["chain_launches"] == 0
    assert a["widest_level"] > 4 * 16  # several blocks of the grid kernel, several passes of the one block


@pytest.mark.parametrize("case", R.DEGENERATE)
def test_degenerate(gpu, case):
    A, f = R.reference(case)
    if A.numRows == 0:  # nothing to factor and nothing launched
        dA = csr_of(A, gpu)
        for chain in CHAINS:
            plan = smfv.Ilu0Plan(dA, chain)
            st = plan.stats()
            assert tuple(plan.factor().shape) == (0,) and st["levels"] == st["launches"] == st["chain_launches"] == 0
        return
    st = three_ways(case, gpu)
    assert st["auto"]["levels"] == 1 and st["auto"]["steps"] == 0


def test_special_values(gpu):
    """Values of +-0.0, 2^+-600 and subnormals, a pivot of exactly +0.0, a NaN
    and a +inf entry: NaN for NaN, everything else bit for bit, under every
    chain setting."""
    A, f = R.reference("special")
    assert np.isfinite(f).mean() >= 0.8 and np.isnan(f).any() and np.isinf(f).any()
    three_ways("special", gpu)


# ---------------------------------------------------------------------------
# in place, re-factor
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band", "long_row"])
def test_in_place(gpu, name):
    """out = A.values on a private copy, the values inside a NaN-filled buffer."""
    A, f = R.reference(name)
    for chain in CHAINS:
        dA = csr_of(A, gpu)
        buf, V = guarded(dA.nnz, gpu)
        V.copy_(dA.values)
        dA.values = V
        assert smfv.Ilu0Plan(dA, chain).factor(out=dA.values) is V
        assert adv.same(read(buf, dA.nnz), f), (name, chain)


def test_refactor_same_plan(gpu):
    """New values on the same plan: the plan holds no values."""
    A, f = R.reference("band")
    A2, f2 = R.reference("band2")
    dA = csr_of(A, gpu)
    plan = dA.ilu0_plan()
    assert dA.ilu0_plan() is plan and dA.ilu0_plan("off") is not plan
    buf, F = guarded(dA.nnz, gpu)
    plan.factor(F)
    assert adv.same(read(buf, dA.nnz), f)
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    plan.factor(F)
    assert adv.same(read(buf, dA.nnz), f2)
    with pytest.raises(ValueError):
        plan.factor(out=F[:-1])


def test_values_changed_with_cached_plans(gpu):
    """An ILU(0) plan cached on a DeviceCSR beside a solve plan and a product
    plan: after an in-place write, values_changed() re-binds every cached
    plan (the ILU(0) plan holds no values: nothing to bind, nothing raised),
    and all three give band2's results."""
    K = 32
    A, f = R.reference("band")
    A2, f2 = R.reference("band2")
    dA = csr_of(A, gpu)
    X = np.array(T.x_full(A.numRows, 3)[:, :K])
    dX = torch.from_numpy(X).to(gpu)
    F = smfv.ilu0(dA)  # caches the ILU(0) plan first, so the plans after it in the cache depend on it
    lower = dA.trsm_plan(K)
    prod = dA.plan(smfv.Variant.ROWWISE, K)
    assert dA.ilu0_plan() in dA._plans.values() and dA.ilu0_plan(thin_rows=16) is not dA.ilu0_plan()
    torch.cuda.synchronize()
    assert adv.same(F.values.cpu().numpy(), f)
    # written through an alias: torch moves dA.values' version counter, so values_changed() is what re-binds
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    dA.values_changed()
    assert lower.bound_version == dA.values_version() == prod.bound_version
    Y = lower.solve(dX)
    P = prod.run(dX, torch.empty_like(dX))
    F2 = dA.ilu0_plan().factor()
    F16 = dA.ilu0_plan(thin_rows=16).factor()
    torch.cuda.synchronize()
    assert adv.same(F2.cpu().numpy(), f2) and adv.same(F16.cpu().numpy(), f2)
    assert dA.ilu0_plan(thin_rows=16).stats()["thin_rows"] == 16
    assert adv.same(Y.cpu().numpy(), T.solve(A2, X, True, False))
    assert adv.same(P.cpu().numpy(), adv.ref_f64(A2, X))
    M = smfv.Ilu0Preconditioner(dA, K, thin_rows=16)
    assert M.plan.stats()["thin_rows"] == 16 and adv.same(M.F.values.cpu().numpy(), f2)


# ---------------------------------------------------------------------------
# with the solves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 32, 40])
def test_factor_then_solves(gpu, K):
    """ilu0(A), then sptrsm lower-unit and upper, equals trsm_ref.solve applied
    twice to the reference factors; Ilu0Preconditioner.apply gives the same."""
    A, f = R.reference("band")
    X, Y = R.applied("band")
    dA = csr_of(A, gpu)
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    F = smfv.ilu0(dA)
    assert isinstance(F, smfv.DeviceCSR) and F.row_ptr is dA.row_ptr and F.col_idx is dA.col_idx
    assert F.h_col_idx is dA.h_col_idx and not F._plans and F.values is not dA.values
    Z = smfv.sptrsm(F, smfv.sptrsm(F, dX, "lower", True), "upper")
    torch.cuda.synchronize()
    assert adv.same(F.values.cpu().numpy(), f)
    assert adv.same(Z.cpu().numpy(), Y[:, :K])
    M = smfv.Ilu0Preconditioner(dA, K)
    Z2 = M.apply(dX)
    torch.cuda.synchronize()
    assert adv.same(Z2.cpu().numpy(), Y[:, :K])
    assert adv.same(dX.cpu().numpy(), X[:, :K]), "X changed"
    W = dX.clone()
    assert M.apply(W, W) is W  # in place
    torch.cuda.synchronize()
    assert adv.same(W.cpu().numpy(), Y[:, :K])


def test_preconditioner_refactor(gpu):
    """After refactor with band2's values, apply gives band2's result: the
    library wrote F.values behind torch's back, so a missed re-bind of the
    solves would give band's."""
    K = 32
    A, _ = R.reference("band")
    A2, f2 = R.reference("band2")
    X, Y = R.applied("band")
    _, Y2 = R.applied("band2")
    assert not np.array_equal(Y, Y2)
    dA = csr_of(A, gpu)
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    M = smfv.Ilu0Preconditioner(dA, K)
    assert adv.same(M.apply(dX).cpu().numpy(), Y[:, :K])
    version = M.F.values._version
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    M.refactor()
    assert M.F.values._version == version  # torch saw no write: only the explicit re-bind helps
    Z = M.apply(dX)
    torch.cuda.synchronize()
    assert adv.same(M.F.values.cpu().numpy(), f2)
    assert adv.same(Z.cpu().numpy(), Y2[:, :K])


# ---------------------------------------------------------------------------
# capture and streams
# ---------------------------------------------------------------------------
def _sequence(dA, K, gpu):
    """factor + both binds + both solves as one function of a stream."""
    M = smfv.Ilu0Preconditioner(dA, K)
    dX = torch.full((dA.m, K), NAN, dtype=torch.float64, device=gpu)
    Yb = torch.full((dA.m, K), NAN, dtype=torch.float64, device=gpu)

    def steps(s):
        M.refactor(s)
        M.apply(dX, Yb, s)
    return M, dX, Yb, steps


def _hip_runtime():
    """The HIP runtime this process already runs on (not a second copy)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def captured_structure(fn):
    """fn(side) captured on a fresh side stream through the runtime's own
    calls (global mode), the graph read back and destroyed without running:
    (nodes, edges, linear) -- linear: no node has two successors or two
    predecessors, and the edges join all nodes into one chain."""
    hip = _hip_runtime()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphDestroy.argtypes = [vp]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = vp()
    assert hip.hipStreamBeginCapture(side.cuda_stream, 0) == 0  # hipStreamCaptureModeGlobal
    try:
        fn(side)
    finally:
        rc = hip.hipStreamEndCapture(side.cuda_stream, ctypes.byref(graph))
    assert rc == 0 and graph.value
    try:
        n, e = sz(0), sz(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
        assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(e)) == 0
        src, dst = (vp * max(e.value, 1))(), (vp * max(e.value, 1))()
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(e)) == 0
        a, b = list(src[:e.value]), list(dst[:e.value])
        linear = e.value == n.value - 1 and len(set(a)) == len(a) and len(set(b)) == len(b)
        return n.value, e.value, linear
    finally:
        hip.hipGraphDestroy(graph)


def test_captured_factor_binds_solves(gpu):
    """Captured once (global capture mode: a hidden allocation, synchronisation
    or null-stream launch is an error), replayed after the values were
    overwritten with band2's; the captured sequence is linear."""
    K = 32
    A, _ = R.reference("band")
    A2, f2 = R.reference("band2")
    X, Y = R.applied("band")
    _, Y2 = R.applied("band2")
    dA = csr_of(A, gpu)
    M, dX, Yb, steps = _sequence(dA, K, gpu)
    torch.cuda.synchronize()
    M.F.values.fill_(NAN)
    launches = M.plan.stats()["launches"] + M.lower.stats()["launches"] + M.upper.stats()["launches"]
    nodes, edges, linear = captured_structure(steps)
    print("ILU0 captured graph:", nodes, "nodes,", edges, "edges;", launches, "factor and solve launches")
    assert nodes >= launches + 2 and linear, "the captured sequence has parallel branches"
    g, side = capture(steps)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Yb).all()) and bool(torch.isnan(M.F.values).all()), "the capture executed"
    dX.copy_(torch.from_numpy(np.array(X[:, :K])))
    g.replay()
    torch.cuda.synchronize()
    assert adv.same(Yb.cpu().numpy(), Y[:, :K])
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    Yb.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    assert adv.same(M.F.values.cpu().numpy(), f2)
    assert adv.same(Yb.cpu().numpy(), Y2[:, :K]), "the replay factors and binds again"
    del g


def test_stream_order(gpu):
    """The same sequence eagerly on a side stream with no device-wide sync."""
    K = 32
    A, _ = R.reference("band")
    A2, _ = R.reference("band2")
    X, _ = R.applied("band")
    _, Y2 = R.applied("band2")
    dA = csr_of(A, gpu)
    M, dX, Yb, steps = _sequence(dA, K, gpu)
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    Xsrc = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    s = torch.cuda.Stream()
    Yout = in_stream_order(s, dX, Xsrc, steps, Yb, gpu)
    torch.cuda.synchronize()
    assert adv.same(Yout.cpu().numpy(), Y2[:, :K])


# ---------------------------------------------------------------------------
# refusals (each returns before any allocation or launch: no plan is made)
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    dA = shared_csr("band", gpu)
    m = dA.m
    rp = dA.h_row_ptr.ctypes.data_as(IP)
    h = ctypes.c_void_p()

    def create(ci, flags):
        return lib.smfv_ilu0_plan_create(ctypes.byref(h), m, dA.nnz, rp, ci.ctypes.data_as(IP), flags)
    ci = dA.h_col_idx.copy()
    ci[ci.size // 3] = m
    assert create(ci, 0) == -1 and not h.value and f"column index {m} " in lib.smfv_last_error().decode()
    assert create(dA.h_col_idx, 4 | 8) == -1 and not h.value
    assert create(dA.h_col_idx, 1) == -1 and not h.value and "unknown flags" in lib.smfv_last_error().decode()
    B = T.band()  # duplicated diagonal entries
    with pytest.raises(SmfvError, match="more than once"):
        smfv.Ilu0Plan(csr_of(B, gpu))
    with pytest.raises(SmfvError, match="more than once"):
        smfv.ilu0(csr_of(B, gpu))
    C = adv.adv_pattern(300, 300, 2)
    with pytest.raises(SmfvError):
        smfv.Ilu0Plan(csr_of(C, gpu))
    with pytest.raises(ValueError, match="square"):
        smfv.Ilu0Plan(csr_of(adv.adv_pattern(300, 200, 2), gpu))
    with pytest.raises(ValueError):
        smfv.Ilu0Plan(dA, chain="both")
    # the device is still usable
    A, f = R.reference("band")
    F = smfv.Ilu0Plan(dA).factor()
    torch.cuda.synchronize()
    assert adv.same(F.cpu().numpy(), f)
    plan = smfv.Ilu0Plan(dA, "off")
    call("smfv_ilu0_plan_factor", plan._plan, dA.values.data_ptr(), F.data_ptr(), stream_handle(None))
    torch.cuda.synchronize()
    assert adv.same(F.cpu().numpy(), f)
