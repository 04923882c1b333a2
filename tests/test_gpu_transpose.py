"""Y = A^T X through a plan (SMFV_PLAN_TRANSPOSE, SpmmPlan(..., transpose=True),
spmm_t) on every path a plan can take.

The contract (include/smfv.h): Y[c] sums values[j] * X[row(j)] over the CSR
entries j of A with col_idx[j] == c in ascending j -- the reference's
sequential loop on the CSR of A^T obtained by a STABLE sort of A's entries by
column.  The reference here is adversarial.ref_f64 (a plain numpy loop) on the
test's own numpy transposition of A, never the library's.

The input is built on the output side, because adversarial.adv_values needs
the length-1 rows adv_pattern has and its transpose has not: B (n_out x m_in)
= adv_pattern with sorted rows gets adv_values' special values, A = B^T
(stable) with every row shuffled (pattern and values together), At = A^T
(stable) is what the plan must reproduce.  At differs from B in the order of
repeated entries, so the tie order of a stable sort is under test.

Bit-exact paths are compared with adversarial.same (NaN for NaN, bits
elsewhere); NONZERO on the merge path and FMA with the project's tolerance,
1e-12 x sum|a||x| + 1e-300.  Every case asserts through stats() which kernel
its inner plan runs.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
from test_gpu_adversarial import execute, note
from test_gpu_capture import NAN, all_nan, capture, gpu_sleep, in_stream_order, read, sleep_cycles_per_ms, window

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import engine
from sparsematrixmultiplicationmpi_amd._lib import SmfvError, call, lib
from sparsematrixmultiplicationmpi_amd.engine import stream_handle

pytestmark = pytest.mark.gpu
V = smfv.Variant
BITWISE = (V.SEQUENTIAL, V.ROWWISE, V.COLUMNWISE)
SEED = 1
KX = 128
# (n_out, m_in): rows of Y / of A^T, rows of X / of A.  Rectangular both
# ways: n (the X bound of the forward kernels) and m swap roles.
SQ, WIDE, TALL = (3000, 3000), (3000, 2400), (2400, 3000)
SHAPES = [SQ, WIDE, TALL]
SHAPE_IDS = ["3000x3000", "3000x2400", "2400x3000"]
ALPHA, BETA = 1.0 / 3.0, -0.7
IP = ctypes.POINTER(ctypes.c_int)


def _frozen(a):
    a.setflags(write=False)
    return a


def np_transpose(C):
    """The test's own stable transposition: entries sorted by column, ties in CSR order."""
    ci = np.asarray(C.colIndices, np.int64)
    perm = np.argsort(ci, kind="stable")
    rp = np.zeros(C.numCols + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(ci, minlength=C.numCols))
    rows = np.repeat(np.arange(C.numRows), np.diff(np.asarray(C.rowPtr, np.int64)))
    return adv.Csr(C.values[perm], rows[perm].astype(np.int32), rp, C.numCols, C.numRows)


def sort_rows(C):
    ci, va = C.colIndices.copy(), C.values.copy()
    for r in range(C.numRows):
        s, e = int(C.rowPtr[r]), int(C.rowPtr[r + 1])
        o = np.argsort(ci[s:e], kind="stable")
        ci[s:e], va[s:e] = ci[s:e][o], va[s:e][o]
    return adv.Csr(va, ci, C.rowPtr, C.numRows, C.numCols)


def shuffle_rows(C, seed):
    rng = np.random.default_rng(seed)
    ci, va = C.colIndices.copy(), C.values.copy()
    for r in range(C.numRows):
        s, e = int(C.rowPtr[r]), int(C.rowPtr[r + 1])
        o = rng.permutation(e - s)
        ci[s:e], va[s:e] = ci[s:e][o], va[s:e][o]
    return adv.Csr(va, ci, C.rowPtr, C.numRows, C.numCols)


class TProblem:
    """A (m_in x n_out, what the plan gets), X, and At = A^T by the test's own
    stable transposition with its references; computed once, read-only."""

    def __init__(self, A, X, B=None):
        self.A, self.X, self.B = A, _frozen(X), B
        self.At = np_transpose(A)
        self._dev = None

    @functools.cached_property
    def Yref(self):
        return _frozen(adv.ref_f64(self.At, self.X))

    @functools.cached_property
    def Yhi(self):
        return _frozen(adv.ref_hi(self.At, self.X))

    @functools.cached_property
    def scale(self):
        return _frozen(adv.scale_hi(self.At, self.X))

    def with_values(self, values):
        A = self.A
        return TProblem(adv.Csr(values, A.colIndices, A.rowPtr, A.numRows, A.numCols), self.X)

    def csr(self, gpu):
        """A DeviceCSR of the caller's own."""
        A = self.A
        return smfv.DeviceCSR(smfv.SparseMatrix(A.values, A.colIndices, A.rowPtr, A.numRows, A.numCols), gpu)

    def dev(self, gpu):
        if self._dev is None:
            self._dev = (self.csr(gpu), torch.from_numpy(np.array(self.X)).to(gpu))
        return self._dev


@functools.lru_cache(maxsize=None)
def tproblem(shape=SQ, kind="long", finite=False):
    n_out, m_in = shape
    B = sort_rows(adv.adv_pattern(n_out, m_in, SEED, adv.LONG_ROWS if kind == "long" else None))
    X = np.random.default_rng(SEED).uniform(-1, 1, (m_in, KX))
    Bv, Xv, _ = adv.adv_values(B, X, finite_only=finite)
    A = shuffle_rows(np_transpose(Bv), SEED)
    assert (A.numRows, A.numCols) == (m_in, n_out)
    return TProblem(A, Xv, Bv)


@functools.lru_cache(maxsize=None)
def reshuffled(shape, which):
    """tproblem(shape) with A's values permuted (same pattern, same X)."""
    pb = tproblem(shape)
    return pb.with_values(pb.A.values[np.random.default_rng(100 + which).permutation(pb.A.nnz)])


def tplan(v, dA, K, **kw):
    plan = smfv.SpmmPlan(v, dA, K, transpose=True, **kw)
    assert plan.transposed and plan.m_out == dA.n
    return plan


def check_tol(Y, pb, cols):
    ok, worst = adv.within_tol(Y, pb.Yhi[:, cols], pb.scale[:, cols], pb.Yref[:, cols])
    print("TOL worst error / bound", worst)
    return ok


# ---------------------------------------------------------------------------
# the input is what the cases need
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_input_facts(shape):
    pb = tproblem(shape)
    At, A = pb.At, pb.A
    assert (At.numRows, At.numCols) == shape and A.nnz == At.nnz
    lens = np.diff(At.rowPtr)
    assert 58 <= int((lens == 0).sum()) <= 73, int((lens == 0).sum())
    assert int((lens == 1300).sum()) == 1 and int((lens == 700).sum()) == 1 and np.sort(lens)[-3] < 700
    Y = pb.Yref
    assert 0 < np.isnan(Y).mean() < 0.02 and 0 < np.isinf(Y).mean() < 0.02
    # unsorted rows in A, and the tie order matters: the reference on At is not the one on B
    unsorted = sum(bool(np.any(np.diff(A.colIndices[A.rowPtr[r]:A.rowPtr[r + 1]]) < 0)) for r in range(A.numRows))
    assert unsorted > A.numRows // 2
    Yb = adv.ref_f64(pb.B, pb.X)
    nan = np.isnan(Y)
    differ = (np.isnan(Yb) != nan) | (~nan & (adv.bits(Yb) != adv.bits(Y)))
    nrows = int(differ.any(axis=1).sum())
    print("rows whose sum depends on the tie order:", nrows)
    assert nrows >= 69, nrows  # (150-205 with this shuffle's seeds: many rows, whatever the shuffle)


def test_input_facts_short():
    pb = tproblem(SQ, "short")
    lens = np.diff(pb.At.rowPtr)
    assert lens.max() <= 1024 and (lens == 0).any()


# ---------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("K", [3, 33, 32])
def test_untiled(gpu, K, shape):
    """k_rows / k_rows_mh on the plan-owned transposed pattern and values."""
    pb = tproblem(shape)
    dA, dX = pb.dev(gpu)
    for v in BITWISE:
        plan = tplan(v, dA, K, tiles="off")
        st = plan.stats()
        assert not st["tiled"] and st["kernel"] is None, st
        note(f"T untiled K={K} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :K], shape[0], K, gpu), pb.Yref[:, :K]), (K, v)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", ["long", "short"])
def test_spmv_k1(gpu, kind, shape):
    """K = 1: k_spmv_stream (the 1,300-entry row of At keeps the pattern off
    the chunk layout) and k_spmv_chunks."""
    pb = tproblem(shape, kind)
    dA, dX = pb.dev(gpu)
    for v in BITWISE:
        plan = tplan(v, dA, 1)
        st = plan.stats()
        assert st["kernel"] == (None if kind == "long" else "k_spmv_chunks") and st["tiled"] == (kind != "long"), st
        note(f"T k1 {kind} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :1], shape[0], 1, gpu), pb.Yref[:, :1]), (kind, v)
        assert adv.same(execute(plan, dX[:, :1], shape[0], 1, gpu, pad=0), pb.Yref[:, :1]), (kind, v)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("K,pairs", [(32, "off"), (32, "on"), (64, "off")])
@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("tk", ["ws1", "ws2", "ws3"])
def test_ws_tiles(gpu, tk, live, K, pairs, shape):
    """k_rows_ws geometries 1 / 2 / 3, snapshot and live values (both from the
    plan's transposed values), row pairs, the two long rows of At on
    k_rows_list."""
    pb = tproblem(shape)
    dA, dX = pb.dev(gpu)
    for v in BITWISE:
        plan = tplan(v, dA, K, tiles="force", tiled_kernel=tk, live_values=live, row_pairs=pairs)
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["ws_geom"] == int(tk[-1]), st
        assert st["live_values"] == live and (st["paired_rows"] > 0) == (pairs == "on"), st
        assert st["direct_rows"] >= 1, st
        note(f"T ws {tk} live={live} pairs={pairs} K={K} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :K], shape[0], K, gpu), pb.Yref[:, :K]), (v, st)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("live", [False, True])
def test_ws_narrow_window(gpu, live, shape):
    """k_rows_ws NARROW: the 16-column window [16, 32) of a 32-wide X."""
    K, f = 16, 16
    pb = tproblem(shape)
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :32].contiguous()
    for v in BITWISE:
        plan = tplan(v, dA, K, tiles="force", live_values=live)
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["live_values"] == live and st["direct_rows"] >= 1, st
        note(f"T ws narrow live={live} {v.name}", st)
        assert adv.same(execute(plan, dX32[:, f:f + K], shape[0], K, gpu), pb.Yref[:, f:f + K]), (v, st)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("K", [4, 8])
def test_wsn_tiles(gpu, K, shape):
    """k_rows_wsn: the window of 4 / 8 columns of a 32-wide X."""
    f = 32 - K - 4
    pb = tproblem(shape)
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :32].contiguous()
    for v in BITWISE:
        plan = tplan(v, dA, K, tiles="force")
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_wsn" and st["direct_rows"] >= 1, st
        note(f"T wsn K={K} {v.name}", st)
        assert adv.same(execute(plan, dX32[:, f:f + K], shape[0], K, gpu), pb.Yref[:, f:f + K]), (v, st)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("live", [False, True])
def test_misaligned_views_on_tiled_plan(gpu, live, shape):
    """A tiled plan handed X / Y views the tiled kernel cannot take -- an odd
    leading dimension, an odd column offset -- drops to the untiled row
    kernel at execute: that fallback must read the plan's transposed values
    and pattern, not the caller's.  The aligned view first and last."""
    K = 32
    pb = tproblem(shape)
    dA, dXall = pb.dev(gpu)
    plan = tplan(V.ROWWISE, dA, K, tiles="force", live_values=live)
    st = plan.stats()
    assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["live_values"] == live, st
    note(f"T views live={live}", st)
    Xeven = dXall[:, :40].contiguous()                       # ld 40
    Xodd = torch.empty((shape[1], 41), dtype=torch.float64, device=gpu)  # ld 41
    Xodd[:, :40] = Xeven
    for Xb, f, g, padw in ((Xeven, 0, 0, 2), (Xeven, 1, 0, 2), (Xodd, 0, 0, 2), (Xodd, 3, 1, 2), (Xeven, 0, 1, 2),
                           (Xeven, 2, 0, 3), (Xeven, 0, 0, 2)):
        cols = slice(f, f + K)
        Y = execute(plan, Xb[:, cols], shape[0], K, gpu, g=g, pad=padw)
        assert adv.same(Y, pb.Yref[:, cols]), (f, g, padw, Xb.stride(0))


def test_nonzero_merge_path(gpu):
    """NONZERO, tiles="off": the merge path over the transposed pattern, K = 8, within the tolerance."""
    K = 8
    for shape in SHAPES:
        pb = tproblem(shape)
        dA, dX = pb.dev(gpu)
        plan = tplan(V.NONZERO, dA, K, tiles="off")
        st = plan.stats()
        assert not st["tiled"], st
        note(f"T merge K={K} {shape}", st)
        Y = execute(plan, dX[:, :K], shape[0], K, gpu)
        assert check_tol(Y, pb, slice(0, K)), shape
        assert np.array_equal(adv.bits(execute(plan, dX[:, :K], shape[0], K, gpu)), adv.bits(Y))


def test_nonzero_tiled_is_bitwise(gpu):
    """NONZERO whose inner plan takes the tiled kernel: bit-identical, as without the flag."""
    K = 32
    for shape in SHAPES:
        pb = tproblem(shape)
        dA, dX = pb.dev(gpu)
        plan = tplan(V.NONZERO, dA, K, tiles="force")
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws", st
        note(f"T nonzero tiled {shape}", st)
        assert adv.same(execute(plan, dX[:, :K], shape[0], K, gpu), pb.Yref[:, :K]), shape


def test_fma_opt_in(gpu):
    """SMFV_PLAN_FMA on the finite input: within the tolerance."""
    K = 32
    pb = tproblem(SQ, finite=True)
    dA, dX = pb.dev(gpu)
    plan = tplan(V.ROWWISE, dA, K, tiles="force", fma=True)
    st = plan.stats()
    assert st["tiled"] and st["kernel"] == "k_rows_ws", st
    note("T fma K=32", st)
    assert check_tol(execute(plan, dX[:, :K], SQ[0], K, gpu), pb, slice(0, K))


# ---------------------------------------------------------------------------
# degenerate shapes
# ---------------------------------------------------------------------------
def _holes(m, n, seed):
    """Empty rows and empty columns: every 3rd row empty, columns = 2 (mod 5) unused."""
    rng = np.random.default_rng(seed)
    cols_ok = np.array([c for c in range(n) if c % 5 != 2])
    rows = [rng.choice(cols_ok, 0 if r % 3 == 1 else int(rng.integers(1, 9))) for r in range(m)]
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return adv.Csr(rng.uniform(-1, 1, int(rp[-1])), np.concatenate(rows).astype(np.int32), rp, m, n)


DEGENERATE = {"1x500": lambda: adv.adv_degenerate(1, 500, SEED), "500x1": lambda: adv.adv_degenerate(500, 1, SEED),
              "1x1": lambda: adv.adv_degenerate(1, 1, SEED), "2000x3": lambda: adv.adv_degenerate(2000, 3, SEED),
              "holes_300x211": lambda: _holes(300, 211, 7),
              "empty_40x30": lambda: adv.Csr(np.zeros(0), np.zeros(0, np.int32), np.zeros(41, np.int32), 40, 30)}


@pytest.mark.parametrize("case", list(DEGENERATE))
def test_degenerate_shapes(gpu, case):
    """A^T of one 300-entry row, of one column, of one entry, of three
    columns, of a matrix with empty rows and empty columns and of one with
    no entry at all, at K = 1 / 4 /
    8 / 32, forced and automatic plans, every variant, into a NaN-filled Y:
    an empty column of A is written as +0.0."""
    A = DEGENERATE[case]()
    m, n = A.numRows, A.numCols
    X = np.random.default_rng(SEED).uniform(-1, 1, (m, 32))
    if m >= 3:
        X[-1] = -0.0
    pb = TProblem(A, X)
    if case == "holes_300x211":
        empty = np.diff(pb.At.rowPtr) == 0
        assert empty.any() and (np.diff(A.rowPtr) == 0).any()
        assert (pb.Yref[empty] == 0).all() and not np.signbit(pb.Yref[empty]).any()
    dA, dX = pb.dev(gpu)
    for K in (1, 4, 8, 32):
        for tiles in ("force", "auto"):
            for v in V:
                plan = tplan(v, dA, K, tiles=tiles)
                st = plan.stats()
                note(f"T degenerate {case} K={K} {tiles} {v.name}", st)
                Y = execute(plan, dX[:, :K], n, K, gpu)
                if v == V.NONZERO and not st["tiled"]:
                    assert check_tol(Y, pb, slice(0, K)), (K, tiles)
                else:
                    assert adv.same(Y, pb.Yref[:, :K]), (K, tiles, v, st)


# ---------------------------------------------------------------------------
# values contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"tiles": "off"}, {"tiles": "force"}, {"tiles": "force", "live_values": True}],
                         ids=["untiled", "snapshot", "live"])
def test_values_contract(gpu, kw):
    """Every transposed plan -- untiled and live ones too -- computes from the
    values of its last bind: new values in place are followed after a bind and
    not before; another values tensor is refused before any launch."""
    K, shape = 32, WIDE
    pb, pb2 = tproblem(shape), reshuffled(shape, 1)
    _, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    dA = pb.csr(gpu)
    plan = tplan(V.ROWWISE, dA, K, **kw)
    st = plan.stats()
    assert st["tiled"] == (kw["tiles"] == "force") and st["live_values"] == bool(kw.get("live_values")), st
    assert adv.same(execute(plan, dX, shape[0], K, gpu), pb.Yref[:, :K])
    dA.values.copy_(torch.from_numpy(pb2.A.values))  # in place: same address
    assert adv.same(execute(plan, dX, shape[0], K, gpu), pb.Yref[:, :K]), "no re-bind: the bound values still"
    plan.bind_values()
    assert adv.same(execute(plan, dX, shape[0], K, gpu), pb2.Yref[:, :K]), "after the re-bind"
    # a different values tensor: refused, Y untouched
    mine = dA.values
    dA.values = mine.clone()
    Yb, Yw = window(shape[0], K, gpu)
    with pytest.raises(RuntimeError, match="not bound"):
        plan.run(dX, Yw)
    assert all_nan(Yb)
    dA.values = mine
    assert adv.same(execute(plan, dX, shape[0], K, gpu), pb2.Yref[:, :K])


def test_execute_before_any_bind_is_refused(gpu):
    """The C call: a transposed plan that was never bound refuses execute
    (SMFV_ERR_INVALID) before anything is launched, also an untiled one."""
    K, shape = 32, WIDE
    pb = tproblem(shape)
    dA, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    h = ctypes.c_void_p()
    call("smfv_plan_create", ctypes.byref(h), int(V.ROWWISE), dA.m, dA.n, dA.nnz, dA.h_row_ptr.ctypes.data_as(IP),
         dA.h_col_idx.ctypes.data_as(IP), K, engine.PLAN_TRANSPOSE | engine.PLAN_NO_TILES)
    try:
        flag = ctypes.c_int(0)
        call("smfv_plan_is_transposed", h, ctypes.byref(flag))
        assert flag.value == 1
        Yb, Yw = window(shape[0], K, gpu)
        rc = lib.smfv_plan_execute(h, None, None, dA.values.data_ptr(), dX.data_ptr(), K, Yw.data_ptr(), Yw.stride(0),
                                   stream_handle(None))
        assert rc == -1 and all_nan(Yb)
        # bound: row_ptr / col_idx may be NULL
        call("smfv_plan_bind_values", h, dA.values.data_ptr(), stream_handle(None))
        call("smfv_plan_execute", h, None, None, dA.values.data_ptr(), dX.data_ptr(), K, Yw.data_ptr(), Yw.stride(0),
             stream_handle(None))
        assert adv.same(read(Yb, K), pb.Yref[:, :K])
    finally:
        call("smfv_plan_destroy", h)


def test_device_csr_plan_rebinds_itself(gpu):
    """DeviceCSR.plan(..., transpose=True) / spmm_t: cached beside the forward
    plan, re-bound when `values` changed since its bind."""
    K, shape = 32, TALL
    pb, pb2 = tproblem(shape), reshuffled(shape, 1)
    _, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    dA = pb.csr(gpu)
    p = dA.plan(V.ROWWISE, K, transpose=True)
    fwd = dA.plan(V.ROWWISE, K)
    assert p.transposed and not fwd.transposed and p is not fwd and dA.plan(V.ROWWISE, K, transpose=True) is p
    assert not smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="off").transposed
    Y = smfv.spmm_t(V.ROWWISE, dA, dX)
    torch.cuda.synchronize()
    assert Y.shape == (shape[0], K) and adv.same(Y.cpu().numpy(), pb.Yref[:, :K])
    dA.values.copy_(torch.from_numpy(pb2.A.values))
    Y = smfv.spmm_t(V.ROWWISE, dA, dX)
    torch.cuda.synchronize()
    assert adv.same(Y.cpu().numpy(), pb2.Yref[:, :K])
    with pytest.raises(ValueError):
        p.run(dX[:shape[0]], Y)  # X must be (A.m, K), not (A.n, K)


# ---------------------------------------------------------------------------
# alpha / beta
# ---------------------------------------------------------------------------
def expected(S, Y0, alpha=ALPHA, beta=BETA):
    with np.errstate(all="ignore"):
        return alpha * S + beta * Y0 if beta != 0 else alpha * S


@pytest.mark.parametrize("K,kw,mode", [(32, {"tiles": "force", "axpby": True}, "fused"),
                                       (3, {"tiles": "off", "axpby": True}, "fused"),
                                       (32, {"tiles": "force", "axpby": "two_pass"}, "two_pass")],
                         ids=["fused-tiled-K32", "fused-untiled-K3", "two_pass-K32"])
def test_axpby(gpu, K, kw, mode):
    """Y <- alpha A^T X + beta Y: the header's formula on the reference sums;
    beta = 0 on a NaN-filled Y; alpha = 1, beta = 0 gives the bits of run."""
    shape = WIDE
    pb = tproblem(shape)
    dA, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    S = pb.Yref[:, :K]
    Y0 = np.random.default_rng(7).uniform(-1, 1, (shape[0], K))
    Y0[0::11, 0::3] = -0.0
    Y0[2::11, :] = np.inf
    Y0[4::11, :] = np.nan
    plan = tplan(V.ROWWISE, dA, K, **kw)
    st = plan.stats()
    assert plan.epilogue_mode == mode and st["tiled"] == (kw["tiles"] == "force"), (plan.epilogue_mode, st)
    note(f"T axpby {mode} K={K}", st)

    def go(y0, alpha, beta):
        Yb, Yw = window(shape[0], K, gpu)
        if y0 is not None:
            Yw.copy_(torch.from_numpy(y0))
        plan.run_axpby(dX, Yw, alpha, beta)
        return read(Yb, K)
    assert adv.same(go(Y0, ALPHA, BETA), expected(S, Y0)), mode
    assert adv.same(go(None, ALPHA, 0.0), expected(S, None, ALPHA, 0.0)), "beta = 0 reads no Y"
    assert adv.same(go(None, 1.0, 0.0), execute(plan, dX, shape[0], K, gpu)), "alpha = 1, beta = 0"
    assert adv.same(go(None, 1.0, 0.0), S)


# ---------------------------------------------------------------------------
# capture and streams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"tiles": "force"}, {"tiles": "off"}], ids=["snapshot", "untiled"])
def test_captured_bind_execute(gpu, kw):
    """bind + execute captured once through the C calls; the gather runs at
    every replay: values changed in place and a new X give the new reference."""
    K, shape = 32, SQ
    pb, pb2 = tproblem(shape), reshuffled(shape, 2)
    _, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    dA = pb.csr(gpu)
    plan = tplan(V.ROWWISE, dA, K, **kw)
    note(f"T captured bind {kw}", plan.stats())
    Yb, Yw = window(shape[0], K, gpu)
    va = dA.values

    def steps(s):
        call("smfv_plan_bind_values", plan._plan, va.data_ptr(), stream_handle(s))
        call("smfv_plan_execute", plan._plan, None, None, va.data_ptr(), dX.data_ptr(), dX.stride(0), Yw.data_ptr(),
             Yw.stride(0), stream_handle(s))
    g, side = capture(steps)
    assert all_nan(Yb), "the capture executed"
    g.replay()
    assert adv.same(read(Yb, K), pb.Yref[:, :K])
    va.copy_(torch.from_numpy(pb2.A.values))
    dX.copy_(dXall[:, K:2 * K])
    Yb.fill_(NAN)
    g.replay()
    assert adv.same(read(Yb, K), pb2.Yref[:, K:2 * K]), "the replay re-gathers"
    # afterwards the plan serves eager calls with the values bound last
    torch.cuda.synchronize()
    Yb.fill_(NAN)
    plan.run(dX, Yw)
    assert adv.same(read(Yb, K), pb2.Yref[:, K:2 * K])
    del g


def test_capture_two_pass_axpby(gpu):
    """run_axpby of a two-pass transposed plan (its kernels into the inner
    plan's scratch, then k_axpby), captured and replayed on two X."""
    K, shape = 32, TALL
    pb = tproblem(shape)
    dA, dXall = pb.dev(gpu)
    plan = tplan(V.ROWWISE, dA, K, tiles="force", axpby="two_pass")
    assert plan.epilogue_mode == "two_pass" and plan.stats()["tiled"], plan.stats()
    dX = dXall[:, :K].contiguous()
    Y0 = np.random.default_rng(7).uniform(-1, 1, (shape[0], K))
    dY0 = torch.from_numpy(Y0).to(gpu)
    Yb, Yw = window(shape[0], K, gpu)
    g, side = capture(lambda s: plan.run_axpby(dX, Yw, ALPHA, BETA, stream=s))
    assert all_nan(Yb), "the capture executed"
    for c0 in (0, K):
        dX.copy_(dXall[:, c0:c0 + K])
        Yw.copy_(dY0)
        g.replay()
        assert adv.same(read(Yb, K), expected(pb.Yref[:, c0:c0 + K], Y0)), c0
    del g


@pytest.mark.parametrize("kw", [{"tiles": "force"}, {"tiles": "off"}], ids=["snapshot", "untiled"])
def test_bound_on_another_stream(gpu, kw):
    """Re-bound on another, busy stream just before an execute on a side
    stream, with no device-wide synchronise in between: the execute waits for
    the bind (the stale values would give the old result)."""
    K, shape = 32, SQ
    pb, want = tproblem(shape), reshuffled(shape, 1)
    _, dXall = pb.dev(gpu)
    Xsrc = dXall[:, :K].contiguous()
    dX = torch.full_like(Xsrc, NAN)
    dA = pb.csr(gpu)
    plan = tplan(V.ROWWISE, dA, K, **kw)
    dA.values.copy_(torch.from_numpy(want.A.values))
    Yb, Yw = window(shape[0], K, gpu)
    s, s_bind = torch.cuda.Stream(), torch.cuda.Stream()

    def launch(st):
        with torch.cuda.stream(s_bind):  # the new values, behind a sleep on another stream
            gpu_sleep(20)
        plan.bind_values(s_bind)
        plan.run(dX, Yw, stream=st)
    Yout = in_stream_order(s, dX, Xsrc, launch, Yb, gpu)
    s_bind.synchronize()
    assert adv.same(read(Yout, K), want.Yref[:, :K])


def test_capture_while_bind_in_flight(gpu):
    """An untiled transposed plan (only the wrapper's own bind to wait for)
    bound on a stream that is still busy: capturing an execute on another
    stream is refused before any launch, the caller's capture (global mode)
    unwinds cleanly, and once the bind stream has drained the same plan
    captures and replays the reference."""
    K, shape = 32, WIDE
    pb = tproblem(shape)
    dA, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    plan = tplan(V.ROWWISE, dA, K, tiles="off")
    Yb, Yw = window(shape[0], K, gpu)
    s_bind = torch.cuda.Stream()
    cycles = int(200 * sleep_cycles_per_ms())
    with pytest.raises(SmfvError, match="still in flight"):
        def busy_bind_then_run(side):
            with torch.cuda.stream(s_bind):
                torch.cuda._sleep(cycles)
            plan.bind_values(s_bind)
            plan.run(dX, Yw, stream=side)
        capture(busy_bind_then_run)
    s_bind.synchronize()
    assert all_nan(Yb)
    g, side = capture(lambda s: plan.run(dX, Yw, stream=s))
    assert all_nan(Yb), "the capture executed"
    g.replay()
    assert adv.same(read(Yb, K), pb.Yref[:, :K])
    del g


# ---------------------------------------------------------------------------
# refusals (each returns before any allocation or launch)
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    pb = tproblem(WIDE)
    dA, _ = pb.dev(gpu)
    with pytest.raises(ValueError):
        smfv.SpmmPlan(V.ROWWISE, dA, 32, rows=(0, 100), transpose=True)
    rp, ci = dA.h_row_ptr.ctypes.data_as(IP), dA.h_col_idx.ctypes.data_as(IP)
    T = engine.PLAN_TRANSPOSE
    h = ctypes.c_void_p()
    assert lib.smfv_plan_create_rows(ctypes.byref(h), int(V.ROWWISE), 0, 100, dA.n, rp, ci, 32, T) == -1 and not h.value
    assert "TRANSPOSE" in lib.smfv_last_error().decode()
    for v in (V.ROWWISE, V.COLUMNWISE, V.NONZERO):
        assert lib.smfv_dist_plan_create_rank(ctypes.byref(h), 2, 0, int(v), 0, 0, dA.m, dA.n, dA.nnz, rp, ci, 32,
                                              T) == -1 and not h.value
        assert "TRANSPOSE" in lib.smfv_last_error().decode()
    # NULL pattern, and a column index outside [0, n)
    assert lib.smfv_plan_create(ctypes.byref(h), int(V.ROWWISE), dA.m, dA.n, dA.nnz, rp, None, 32, T) == -1
    assert lib.smfv_plan_create(ctypes.byref(h), int(V.ROWWISE), dA.m, dA.n, dA.nnz, None, None, 32, T) == -1
    bad = dA.h_col_idx.copy()
    bad[bad.size // 2] = dA.n
    assert lib.smfv_plan_create(ctypes.byref(h), int(V.ROWWISE), dA.m, dA.n, dA.nnz, rp, bad.ctypes.data_as(IP), 32,
                                T) == -1 and not h.value
    assert "column" in lib.smfv_last_error().decode()
