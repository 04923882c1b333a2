"""Triangular solves T Y = X on the GPU (smfv_trsm_plan_*, TrsmPlan, sptrsm):
every result is compared bit for bit (adversarial.same: NaN for NaN, the sign
of zero included) with the sequential substitution of include/smfv.h restated
in numpy (tests/trsm_ref.py: vectorised over K only, never the library).

Inputs, all m = 3000 unless degenerate: `band` (953 / 946 levels, nearly all a
few rows thin, one ~150 rows wide), its variant with 700- and 1,300-entry rows,
`two_level` (64 levels of one row, then one of 2,936), the degenerate shapes
and the special-values case.  Every reference is at least 80 % finite
(asserted where it is built), so no comparison rests on NaN against NaN.  The
three chain settings -- auto, one launch per level, everything in the
one-block kernel -- must give the same bits, and stats() must show the path
each case is for.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
import trsm_ref as T
from test_gpu_capture import NAN, all_nan, capture, gpu_sleep, in_stream_order, read, sleep_cycles_per_ms, window

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import engine
from sparsematrixmultiplicationmpi_amd._lib import SmfvError, call, lib
from sparsematrixmultiplicationmpi_amd.engine import stream_handle

pytestmark = pytest.mark.gpu
IP = ctypes.POINTER(ctypes.c_int)
CHAINS = ("auto", "off", "all")
CHAIN_LANES = 1024


def csr_of(A, gpu):
    return smfv.DeviceCSR(smfv.SparseMatrix(np.array(A.values), np.array(A.colIndices), np.array(A.rowPtr), A.numRows,
                                            A.numCols), gpu)


@functools.lru_cache(maxsize=None)
def shared_csr(name, gpu):
    """The DeviceCSR of a named input, shared and read-only."""
    A = T.special(name == "special_lower")[0] if name.startswith("special") else T.reference(name)[0]
    return csr_of(A, gpu)


@functools.lru_cache(maxsize=None)
def dev_x(m, seed, gpu):
    return torch.from_numpy(np.array(T.x_full(m, seed))).to(gpu)


def team_of(K, vec):
    """Lanes per row, as the library picks them (k_rows' mapping)."""
    need, t = -(-K // vec), 1
    while t < need and t < 64:
        t <<= 1
    return t


def solve(plan, dX, m, K, gpu):
    """Into the window of a NaN-filled buffer; the guard columns must stay NaN."""
    Yb, Yw = window(m, K, gpu)
    plan.solve(dX, Yw)
    return read(Yb, K)


def three_ways(dA, K, uplo, unit, dX, Yref, gpu):
    """auto / off / all against the loop (hence against each other); returns the three stats()."""
    stats = {}
    for chain in CHAINS:
        plan = smfv.TrsmPlan(dA, K, uplo, unit, chain)
        Y = solve(plan, dX, dA.m, K, gpu)
        assert adv.same(Y, Yref), (chain, uplo, unit, K)
        stats[chain] = plan.stats()
    a, o, c = (stats[k] for k in CHAINS)
    print("TRSM", uplo, "unit" if unit else "non-unit", K, {k: (v["launches"], v["chain_launches"]) for k, v in stats.items()})
    assert o["launches"] == o["levels"] == a["levels"] and o["chain_launches"] == 0
    assert c["launches"] == c["chain_launches"] == (1 if dA.m else 0) and c["chain_rows"] == dA.m
    assert c["chain_max_levels"] == c["levels"]
    for st in stats.values():
        assert st["strict_entries"] + st["ignored_entries"] + st["diag_entries"] == dA.nnz and st["plan_bytes"] > 0
    return stats


# ---------------------------------------------------------------------------
# shapes and flags
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8, 32, 33, 128])
@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("uplo", ["lower", "upper"])
def test_band(gpu, uplo, unit, K):
    A, X, Yref = T.reference("band", uplo == "lower", unit)
    dA = shared_csr("band", gpu)
    dX = dev_x(A.numRows, 3, gpu)[:, :K].contiguous()
    stats = three_ways(dA, K, uplo, unit, dX, Yref[:, :K], gpu)
    a, c = stats["auto"], stats["all"]
    assert a["levels"] == (953 if uplo == "lower" else 946) and 148 <= a["widest_level"] <= 152
    # auto: the thin levels ride in chain launches
    assert a["chain_launches"] > 0 and a["chain_max_levels"] > 100 and a["launches"] < a["levels"] // 10
    assert a["diag_entries"] == T.counts(A, uplo == "lower", unit)[2] and (unit or a["diag_entries"] > A.numRows)
    if K >= 32:  # under `all` the widest level takes several passes of the one block
        vec = 2 if K % 2 == 0 else 1
        assert c["widest_level"] > CHAIN_LANES // team_of(K, vec)


@pytest.mark.parametrize("uplo", ["lower", "upper"])
def test_band_long_rows(gpu, uplo):
    """Rows of 700 and 1,300 entries drawn over all columns (many passes of a team over one row)."""
    K = 32
    A, X, Yref = T.reference("band_long", uplo == "lower", False)
    dX = dev_x(A.numRows, 3, gpu)[:, :K].contiguous()
    three_ways(shared_csr("band_long", gpu), K, uplo, False, dX, Yref[:, :K], gpu)


@pytest.mark.parametrize("K", [32, 128])
def test_two_level(gpu, K):
    A, X, Yref = T.reference("two_level", True, False)
    dA = shared_csr("two_level", gpu)
    dX = dev_x(A.numRows, 3, gpu)[:, :K].contiguous()
    stats = three_ways(dA, K, "lower", False, dX, Yref[:, :K], gpu)
    a = stats["auto"]
    assert a["levels"] == 65 and a["widest_level"] == 2936
    assert a["launches"] == 2 and a["chain_launches"] == 1 and a["chain_rows"] == 64 and a["chain_max_levels"] == 64
    team = team_of(K, 2)
    assert a["widest_level"] > 4 * (256 // team)  # the wide level: several blocks of the grid kernel
    assert a["widest_level"] > CHAIN_LANES // team  # and several passes of the one block under `all`
    # upper: nothing above the diagonal but the diagonal itself -- one level, Y = X / d
    _, _, Yup = T.reference("two_level", False, False)
    up = three_ways(dA, K, "upper", False, dX, Yup[:, :K], gpu)
    assert up["auto"]["levels"] == 1 and up["auto"]["strict_entries"] == 0


@pytest.mark.parametrize("K", [3, 32])
@pytest.mark.parametrize("case", T.DEGENERATE)
def test_degenerate(gpu, case, K):
    A, unit = T.degenerate(case)
    m = A.numRows
    dA = csr_of(A, gpu)
    if m == 0:  # nothing to solve and nothing launched: an empty Y comes back
        for uplo in ("lower", "upper"):
            for chain in CHAINS:
                plan = smfv.TrsmPlan(dA, K, uplo, unit, chain)
                Y = plan.solve(torch.empty((0, K), dtype=torch.float64, device=gpu))
                st = plan.stats()
                assert tuple(Y.shape) == (0, K) and st["levels"] == st["launches"] == st["chain_launches"] == 0, st
        return
    dX = dev_x(m, 3, gpu)[:, :K].contiguous()
    for uplo in ("lower", "upper"):
        _, X, Yref = T.reference(case, uplo == "lower", unit)
        stats = three_ways(dA, K, uplo, unit, dX, Yref[:, :K], gpu)
        want = {"m1": 1, "nnz0_unit": 1, "diagonal": 1, "bidiagonal": 300 if uplo == "lower" else 1}[case]
        assert stats["auto"]["levels"] == want, stats["auto"]
        if case == "nnz0_unit":
            assert adv.same(Yref[:, :K], np.array(X[:, :K]))  # Y = X


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("uplo", ["lower", "upper"])
def test_special_values(gpu, uplo):
    """+-inf, NaN, -0.0, 5e-324 and +-1.7e308 rows of X, values of +-0.0 and
    2^+-600, a pivot cancelling to +0.0: NaN for NaN, everything else bit for
    bit (adversarial.same), under every chain setting."""
    K = 32
    A, X, Yref, info = T.special(uplo == "lower")
    dA = shared_csr("special_" + uplo, gpu)
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    ref = Yref[:, :K]
    assert np.isfinite(ref).mean() >= 0.8 and np.isnan(ref).any() and np.isinf(ref).any()
    zeros = ref[ref == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()  # both zeros
    assert (np.abs(ref[ref != 0]) < 2.2e-308).any()  # subnormal results
    assert not np.isfinite(ref[info["zero_pivot_row"]]).any()
    three_ways(dA, K, uplo, False, dX, ref, gpu)


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 33])
def test_views(gpu, K):
    """X and Y as column windows at an odd column offset of wider NaN-filled
    buffers with ldx != ldy (8-byte aligned only: the one-double-per-lane
    kernels), then the same solve in place; nothing outside the window is
    touched, padding is neither read nor written."""
    A, X, Yref = T.reference("band", True, False)
    m = A.numRows
    dA = shared_csr("band", gpu)
    Xb = torch.full((m, K + 7), NAN, dtype=torch.float64, device=gpu)
    Yb = torch.full((m, K + 12), NAN, dtype=torch.float64, device=gpu)
    Xw, Yw = Xb[:, 3:3 + K], Yb[:, 5:5 + K]
    Xw.copy_(dev_x(m, 3, gpu)[:, :K])
    assert Xw.stride(0) != Yw.stride(0) and Xw.data_ptr() % 16 == 8 and Yw.data_ptr() % 16 == 8
    for chain in CHAINS:
        Yb.fill_(NAN)
        plan = smfv.TrsmPlan(dA, K, "lower", False, chain)
        plan.solve(Xw, Yw)
        torch.cuda.synchronize()
        Yh = Yb.cpu().numpy()
        assert adv.same(Yh[:, 5:5 + K], Yref[:, :K]), chain
        assert np.isnan(Yh[:, :5]).all() and np.isnan(Yh[:, 5 + K:]).all(), "Y written outside its window"
        # in place: Y is X
        Zb = Xb.clone()
        Zw = Zb[:, 3:3 + K]
        assert plan.solve(Zw, Zw) is Zw
        torch.cuda.synchronize()
        Zh = Zb.cpu().numpy()
        assert adv.same(Zh[:, 3:3 + K], Yref[:, :K]), ("in place", chain)
        assert np.isnan(Zh[:, :3]).all() and np.isnan(Zh[:, 3 + K:]).all()
    # in place on an aligned, even-strided buffer (two doubles per lane)
    K2 = 32
    Zb, Zw = window(m, K2, gpu)
    Zw.copy_(dev_x(m, 3, gpu)[:, :K2])
    smfv.TrsmPlan(dA, K2).solve(Zw, Zw)
    assert adv.same(read(Zb, K2), Yref[:, :K2])


# ---------------------------------------------------------------------------
# values contract
# ---------------------------------------------------------------------------
def test_values_contract(gpu):
    """The plan computes from the values of its last bind: new values in place
    are followed after a bind and not before; another values tensor is
    refused before any launch."""
    K = 32
    A, X, Yref = T.reference("band", True, False)
    A2, _, Yref2 = T.reference2(True)
    m = A.numRows
    dA = csr_of(A, gpu)
    dX = dev_x(m, 3, gpu)[:, :K].contiguous()
    plan = smfv.TrsmPlan(dA, K)
    assert adv.same(solve(plan, dX, m, K, gpu), Yref[:, :K])
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))  # in place: same address
    assert adv.same(solve(plan, dX, m, K, gpu), Yref[:, :K]), "no re-bind: the bound values still"
    plan.bind_values()
    assert adv.same(solve(plan, dX, m, K, gpu), Yref2[:, :K]), "after the re-bind"
    mine = dA.values
    dA.values = mine.clone()
    Yb, Yw = window(m, K, gpu)
    with pytest.raises(SmfvError, match="not bound"):
        plan.solve(dX, Yw)
    assert all_nan(Yb)
    dA.values = mine
    assert adv.same(solve(plan, dX, m, K, gpu), Yref2[:, :K])


def test_execute_before_any_bind_is_refused(gpu):
    """The C calls: a plan never bound refuses execute (SMFV_ERR_INVALID) before anything is launched."""
    K = 8
    A, X, Yref = T.reference("band", False, False)
    m = A.numRows
    dA = shared_csr("band", gpu)
    dX = dev_x(m, 3, gpu)[:, :K].contiguous()
    h = ctypes.c_void_p()
    call("smfv_trsm_plan_create", ctypes.byref(h), m, dA.nnz, dA.h_row_ptr.ctypes.data_as(IP),
         dA.h_col_idx.ctypes.data_as(IP), K, engine.TRSM_UPPER)
    try:
        Yb, Yw = window(m, K, gpu)
        rc = lib.smfv_trsm_plan_execute(h, dA.values.data_ptr(), dX.data_ptr(), K, Yw.data_ptr(), Yw.stride(0),
                                        stream_handle(None))
        assert rc == -1 and "not bound" in lib.smfv_last_error().decode() and all_nan(Yb)
        call("smfv_trsm_plan_bind_values", h, dA.values.data_ptr(), stream_handle(None))
        assert lib.smfv_trsm_plan_execute(h, dA.values.data_ptr(), dX.data_ptr(), K - 1, Yw.data_ptr(), Yw.stride(0),
                                          stream_handle(None)) == -1  # ldx < K
        assert all_nan(Yb)
        call("smfv_trsm_plan_execute", h, dA.values.data_ptr(), dX.data_ptr(), K, Yw.data_ptr(), Yw.stride(0),
             stream_handle(None))
        assert adv.same(read(Yb, K), Yref[:, :K])
    finally:
        call("smfv_trsm_plan_destroy", h)


def test_device_csr_plan_rebinds_itself(gpu):
    """DeviceCSR.trsm_plan / sptrsm: one cached plan per (K, uplo, unit_diag,
    chain), bound again after an in-place torch write to `values`."""
    K = 32
    A, X, Yref = T.reference("band", True, False)
    A2, _, Yref2 = T.reference2(True)
    dA = csr_of(A, gpu)
    dX = dev_x(A.numRows, 3, gpu)[:, :K].contiguous()
    p = dA.trsm_plan(K)
    assert dA.trsm_plan(K) is p and dA.trsm_plan(K, "upper") is not p and dA.trsm_plan(K, unit_diag=True) is not p
    Y = smfv.sptrsm(dA, dX)
    torch.cuda.synchronize()
    assert Y.shape == (A.numRows, K) and adv.same(Y.cpu().numpy(), Yref[:, :K])
    Yu = smfv.sptrsm(dA, dX, uplo="upper", unit_diag=True)
    torch.cuda.synchronize()
    assert adv.same(Yu.cpu().numpy(), T.reference("band", False, True)[2][:, :K])
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))  # an in-place torch write: same address, new version
    Y = smfv.sptrsm(dA, dX)
    torch.cuda.synchronize()
    assert adv.same(Y.cpu().numpy(), Yref2[:, :K])
    with pytest.raises(ValueError):
        p.solve(dX[:100], Y)


# ---------------------------------------------------------------------------
# capture and streams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["auto", "off"])
def test_captured_bind_solve(gpu, chain):
    """bind + solve captured once (global capture mode: a hidden allocation,
    synchronisation or null-stream launch is an error) through the C calls;
    replayed on new X contents and new values."""
    K = 32
    A, X, Yref = T.reference("band", True, False)
    A2, _, Yref2 = T.reference2(True)
    m = A.numRows
    dA = csr_of(A, gpu)
    dXall = dev_x(m, 3, gpu)
    dX = dXall[:, :K].contiguous()
    plan = smfv.TrsmPlan(dA, K, chain=chain)
    Yb, Yw = window(m, K, gpu)
    va = dA.values

    def steps(s):
        call("smfv_trsm_plan_bind_values", plan._plan, va.data_ptr(), stream_handle(s))
        call("smfv_trsm_plan_execute", plan._plan, va.data_ptr(), dX.data_ptr(), dX.stride(0), Yw.data_ptr(),
             Yw.stride(0), stream_handle(s))
    g, side = capture(steps)
    assert all_nan(Yb), "the capture executed"
    g.replay()
    assert adv.same(read(Yb, K), Yref[:, :K])
    va.copy_(torch.from_numpy(np.array(A2.values)))
    dX.copy_(dXall[:, K:2 * K])
    Yb.fill_(NAN)
    g.replay()
    assert adv.same(read(Yb, K), Yref2[:, K:2 * K]), "the replay binds again"
    torch.cuda.synchronize()
    Yb.fill_(NAN)
    plan.solve(dX, Yw)  # afterwards the plan serves eager calls with the values bound last
    assert adv.same(read(Yb, K), Yref2[:, K:2 * K])
    del g


def test_bound_on_another_stream(gpu):
    """Bound again on another, busy stream just before an eager solve on a
    side stream, with no device-wide synchronise in between: the solve waits
    for the bind (the stale values would give the old result)."""
    K = 32
    A, X, Yref = T.reference("band", True, False)
    A2, _, Yref2 = T.reference2(True)
    m = A.numRows
    dA = csr_of(A, gpu)
    Xsrc = dev_x(m, 3, gpu)[:, :K].contiguous()
    dX = torch.full_like(Xsrc, NAN)
    plan = smfv.TrsmPlan(dA, K)
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    Yb, Yw = window(m, K, gpu)
    s, s_bind = torch.cuda.Stream(), torch.cuda.Stream()

    def launch(st):
        with torch.cuda.stream(s_bind):
            gpu_sleep(20)
        plan.bind_values(s_bind)
        plan.solve(dX, Yw, stream=st)
    Yout = in_stream_order(s, dX, Xsrc, launch, Yb, gpu)
    s_bind.synchronize()
    assert adv.same(read(Yout, K), Yref2[:, :K])


def test_capture_while_bind_in_flight(gpu):
    """Bound on a stream that is still busy: capturing a solve on another
    stream is refused before any launch, the caller's capture (global mode)
    unwinds cleanly, and once the bind stream has drained the same plan
    captures and replays the reference."""
    K = 32
    A, X, Yref = T.reference("band", True, False)
    m = A.numRows
    dA = csr_of(A, gpu)
    dX = dev_x(m, 3, gpu)[:, :K].contiguous()
    plan = smfv.TrsmPlan(dA, K)
    Yb, Yw = window(m, K, gpu)
    s_bind = torch.cuda.Stream()
    cycles = int(200 * sleep_cycles_per_ms())
    with pytest.raises(SmfvError, match="still in flight"):
        def busy_bind_then_solve(side):
            with torch.cuda.stream(s_bind):
                torch.cuda._sleep(cycles)
            plan.bind_values(s_bind)
            plan.solve(dX, Yw, stream=side)
        capture(busy_bind_then_solve)
    s_bind.synchronize()
    assert all_nan(Yb)
    g, side = capture(lambda s: plan.solve(dX, Yw, stream=s))
    assert all_nan(Yb), "the capture executed"
    g.replay()
    assert adv.same(read(Yb, K), Yref[:, :K])
    del g


# ---------------------------------------------------------------------------
# refusals (each returns before any allocation or launch: no plan is made)
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    A = T.band()
    m = A.numRows
    dA = shared_csr("band", gpu)
    rp = dA.h_row_ptr.ctypes.data_as(IP)
    h = ctypes.c_void_p()

    def create(ci, K, flags):
        return lib.smfv_trsm_plan_create(ctypes.byref(h), m, dA.nnz, rp, ci.ctypes.data_as(IP), K, flags)
    # a structurally missing diagonal, the first such row named
    ci = dA.h_col_idx.copy()
    r = np.repeat(np.arange(m), np.diff(dA.h_row_ptr))
    for row in (2222, 717):
        ci[(r == row) & (ci == row)] = row + 1
    for flags in (0, engine.TRSM_UPPER):
        assert create(ci, 32, flags) == -1 and not h.value
        msg = lib.smfv_last_error().decode()
        assert "row 717 " in msg and "diagonal" in msg, msg
    assert create(ci, 32, engine.TRSM_UNIT_DIAG) == 0 and h.value  # ... and legal with UNIT_DIAG
    call("smfv_trsm_plan_destroy", h)
    h = ctypes.c_void_p()
    # a column >= m, K = 0, both chain flags
    ci = dA.h_col_idx.copy()
    ci[ci.size // 3] = m
    assert create(ci, 32, 0) == -1 and not h.value and f"column index {m} " in lib.smfv_last_error().decode()
    assert create(dA.h_col_idx, 0, 0) == -1 and not h.value and "K = 0" in lib.smfv_last_error().decode()
    assert create(dA.h_col_idx, 32, engine.TRSM_NO_CHAIN | engine.TRSM_CHAIN_ALL) == -1 and not h.value
    with pytest.raises(SmfvError, match="K = 0"):
        smfv.TrsmPlan(dA, 0)
    with pytest.raises(ValueError):
        smfv.TrsmPlan(dA, 32, uplo="both")
    # the Python surface refuses a non-square matrix and a wrong X shape
    B = adv.adv_pattern(300, 200, 2)
    with pytest.raises(ValueError, match="square"):
        smfv.TrsmPlan(csr_of(B, gpu), 8, unit_diag=True)
    with pytest.raises(ValueError):
        smfv.TrsmPlan(dA, 8).solve(torch.zeros((m, 9), dtype=torch.float64, device=gpu))
