"""The reordering family on the GPU (smfv_reorder_plan_*, ReorderedCSR,
Ilu0Preconditioner(reorder=...)): every comparison is bit for bit through an
int64 view (NaN payloads and the sign of zero included), against numpy fancy
indexing for the row kernel and against the numpy loops of tests/ilu0_ref.py
and tests/trsm_ref.py run on the host-renumbered matrix (tests/reorder_ref.py,
never the library) for the factorisation and the solves.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
import ilu0_ref as I
import reorder_ref as R
import trsm_ref as T
from test_gpu_adversarial import problem
from test_gpu_capture import NAN, capture, in_stream_order

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd._lib import SmfvError, call, lib
from sparsematrixmultiplicationmpi_amd.engine import REORDER_STORE_NT, REORDER_TO_NEW, REORDER_TO_OLD, stream_handle

pytestmark = pytest.mark.gpu
IP = ctypes.POINTER(ctypes.c_int)
GUARD = 8  # NaN rows' worth of doubles on each side of a buffer


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def csr_of(A, gpu):
    return smfv.DeviceCSR(smfv.SparseMatrix(np.array(A.values), np.array(A.colIndices), np.array(A.rowPtr), A.numRows,
                                            A.numCols), gpu)


class RowsPlan:
    """smfv_reorder_plan_* for rows only (nnz = 0, no vperm), through the C ABI."""

    def __init__(self, perm):
        self.perm = np.ascontiguousarray(perm, np.int32)
        self.h = ctypes.c_void_p()
        call("smfv_reorder_plan_create", ctypes.byref(self.h), self.perm.size, 0, self.perm.ctypes.data_as(IP), None)

    def rows(self, direction, X, ldx, K, Y, ldy, stream=None):
        return lib.smfv_reorder_plan_rows(self.h, direction, X, ldx, K, Y, ldy, stream_handle(stream))

    def __del__(self):
        lib.smfv_reorder_plan_destroy(self.h)


def expected(direction, perm, X):
    """numpy fancy indexing: TO_NEW Y[i] = X[perm[i]]; TO_OLD Y[perm[i]] = X[i]."""
    if direction == REORDER_TO_NEW:
        return X[perm]
    Y = np.empty_like(X)
    Y[perm] = X
    return Y


def special_x(m, K):
    """Rows of tests/adversarial.py's special X (whole rows of +-inf, NaN,
    +-0.0, subnormals, +-1.7e308 among uniform values), then NaNs with distinct
    payloads -- quiet and signalling, both signs --, -0.0 and a subnormal
    scattered over it, every one a bit pattern of its own."""
    Xs = problem().X
    special = sorted(problem().info["x_special"].values())
    rows = (special + [r for r in range(Xs.shape[0]) if r not in special])[:m]
    X = np.ascontiguousarray(Xs[np.sort(rows)][:, :K]).copy()
    v = X.reshape(-1).view(np.uint64)
    n = v.size
    for k in range(0, n, 5):
        v[k] = (0x7ff8000000000000, 0x7ff0000000000000, 0xfff8000000000000, 0xfff0000000000000)[k // 5 % 4] | (k + 1)
    if n > 7:
        v[3], v[7] = 0x8000000000000000, 0x0000000000000003
    return X


def run_rows(plan, direction, Xh, K, gpu, ldx, ldy, shift=0, nt=False):
    """One execution with X and Y as windows of NaN-filled flat buffers:
    leading dimensions ldx / ldy >= K, both views `shift` doubles off a
    16-byte boundary, a guard band before and after.  The padding and the
    guards must still be NaN afterwards; X must be unchanged."""
    m = Xh.shape[0]
    g = GUARD * max(ldx, ldy) + 2
    xb = torch.full((g + m * ldx + g,), NAN, dtype=torch.float64, device=gpu)
    yb = torch.full((g + m * ldy + g,), NAN, dtype=torch.float64, device=gpu)
    base = 2 * ((g + 1) // 2) - 2 + shift  # even + shift: torch allocations are 16-byte aligned
    Xv = xb[base:base + m * ldx].view(m, ldx)[:, :K]
    Yv = yb[base:base + m * ldy].view(m, ldy)[:, :K]
    Xv.copy_(torch.from_numpy(Xh))
    x_before = xb.cpu().numpy().copy()
    assert (Xv.data_ptr() % 16 == 0) == (shift % 2 == 0) and (Yv.data_ptr() % 16 == 0) == (shift % 2 == 0)
    rc = plan.rows(direction | (REORDER_STORE_NT if nt else 0), Xv.data_ptr(), ldx, K, Yv.data_ptr(), ldy)
    assert rc == 0, lib.smfv_last_error()
    torch.cuda.synchronize()
    yh = yb.cpu().numpy()
    win = np.zeros(yh.size, bool)
    idx = base + (np.arange(m)[:, None] * ldy + np.arange(K)[None, :]).reshape(-1)
    win[idx] = True
    assert np.isnan(yh[~win]).all(), "written outside the K columns of Y"
    assert np.array_equal(bits(xb.cpu().numpy()), bits(x_before)), "X changed"
    return yh[idx].reshape(m, K)


# ---------------------------------------------------------------------------
# k_permute_rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32, 40, 128])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 953])
def test_rows(gpu, m, K):
    """Both directions against numpy fancy indexing: contiguous (16-byte
    accesses at even K), ld > K with the padding and a guard band still NaN,
    both views one double off alignment (the 8-byte path at even K too),
    non-temporal stores, and to_old(to_new(X)) == X.  X holds NaNs with
    distinct payloads, +-0.0, subnormals and +-inf."""
    perm = np.random.default_rng(m * 131 + K).permutation(m).astype(np.int32)
    plan = RowsPlan(perm)
    X = special_x(m, K)
    nan = bits(X)[np.isnan(X)]
    assert nan.size >= m * K // 5 and np.unique(nan).size >= min(nan.size, m * K // 5)  # distinct payloads
    for direction in (REORDER_TO_NEW, REORDER_TO_OLD):
        want = expected(direction, perm, X)
        for ldx, ldy, shift, nt in ((K, K, 0, False), (K + 6, K + 2, 0, False), (K + 3, K + 5, 0, False),
                                    (K + 2, K + 2, 1, False), (K, K, 0, True), (K + 1, K + 4, 1, True)):
            got = run_rows(plan, direction, X, K, gpu, ldx, ldy, shift, nt)
            assert same_bits(got, want), (direction, ldx, ldy, shift, nt)
    there = run_rows(plan, REORDER_TO_NEW, X, K, gpu, K, K)
    assert same_bits(run_rows(plan, REORDER_TO_OLD, there, K, gpu, K, K), X)


@pytest.fixture(scope="module")
def big_buffer(gpu):
    """One 5 GB buffer for the large-offset cases (allocated once, freed at the end)."""
    try:
        buf = torch.empty(BIG_M * BIG_LD, dtype=torch.float64, device=gpu)
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"cannot allocate {BIG_M * BIG_LD * 8 / 1e9:.1f} GB of device memory: {e}")
    yield buf
    del buf
    torch.cuda.empty_cache()


BIG_M, BIG_LD, BIG_F = 70, 8_950_000, 6  # row * ld * 8 passes 2^32 from row 60 on; the window starts at column 6


@pytest.mark.parametrize("direction", [REORDER_TO_NEW, REORDER_TO_OLD])
def test_large_offsets(gpu, big_buffer, direction):
    """m = 70 with a leading dimension of 8.95 million doubles: the last ten
    rows lie beyond 4 GiB.  First X is the column window of the large buffer
    (the gather's row * ldx), then Y (the store's row * ldy).  Only the touched
    rows are initialised and compared; a guard of two columns on each side of
    Y's window must stay NaN."""
    K = 32
    assert 59 * BIG_LD * 8 < 1 << 32 <= 60 * BIG_LD * 8 and BIG_LD % 2 == 0
    perm = np.random.default_rng(70).permutation(BIG_M).astype(np.int32)
    plan = RowsPlan(perm)
    X = special_x(BIG_M, K)
    want = expected(direction, perm, X)
    big = big_buffer.view(BIG_M, BIG_LD)
    # X in the large buffer
    Xv = big[:, BIG_F:BIG_F + K]
    Xv.copy_(torch.from_numpy(X))
    Y = torch.full((BIG_M, K), NAN, dtype=torch.float64, device=gpu)
    assert plan.rows(direction, Xv.data_ptr(), BIG_LD, K, Y.data_ptr(), K) == 0, lib.smfv_last_error()
    torch.cuda.synchronize()
    assert same_bits(Y.cpu().numpy(), want)
    # Y in the large buffer
    Yw = big[:, BIG_F - 2:BIG_F + K + 2]
    Yw.fill_(NAN)
    Yv = big[:, BIG_F:BIG_F + K]
    Xs = torch.from_numpy(X).to(gpu)
    assert plan.rows(direction, Xs.data_ptr(), K, K, Yv.data_ptr(), BIG_LD) == 0, lib.smfv_last_error()
    torch.cuda.synchronize()
    got = Yw.cpu().numpy()
    assert np.isnan(got[:, :2]).all() and np.isnan(got[:, -2:]).all(), "written outside Y's window"
    assert same_bits(got[:, 2:-2], want)


# ---------------------------------------------------------------------------
# values, cached plans, the identity
# ---------------------------------------------------------------------------
def test_values_follow(gpu):
    """B.values == A.values[vperm]; after an in-place change of A.values, .B
    and its cached plans follow: an SpMM plan, a solve and an ILU(0) plan."""
    K = 32
    A, A2 = I.band(), I.band2()
    Bh, vperm = R.renumbered("band")
    perm, _, nc = R.ordering("band")
    dA = csr_of(A, gpu)
    Rd = dA.reordered()
    assert isinstance(Rd, smfv.ReorderedCSR) and Rd.ncolors == nc and np.array_equal(Rd.perm, perm)
    assert np.array_equal(Rd.vperm, vperm) and np.array_equal(Rd.color, R.ordering("band")[1])
    st = Rd.stats()
    assert (st["m"], st["nnz"]) == (A.numRows, A.nnz) and st["plan_bytes"] >= 4 * (2 * A.numRows + A.nnz)
    B = Rd.B
    assert isinstance(B, smfv.DeviceCSR) and np.array_equal(B.h_row_ptr, Bh.rowPtr) and np.array_equal(B.h_col_idx, Bh.colIndices)
    torch.cuda.synchronize()
    assert same_bits(B.values.cpu().numpy(), np.asarray(A.values)[vperm])
    X = np.array(T.x_full(A.numRows, 3)[:, :K])
    dX = torch.from_numpy(X).to(gpu)
    prod = B.plan(smfv.Variant.ROWWISE, K)
    lower = B.trsm_plan(K)
    ilu = B.ilu0_plan()
    torch.cuda.synchronize()
    assert same_bits(prod.run(dX, torch.empty_like(dX)).cpu().numpy(), adv.ref_f64(Bh, X))
    # an in-place write: torch moves A.values' version, and .B notices
    dA.values.copy_(torch.from_numpy(np.array(A2.values)))
    assert Rd.B is B
    B2h = adv.Csr(np.asarray(A2.values)[vperm], Bh.colIndices, Bh.rowPtr, Bh.numRows, Bh.numCols)
    P = prod.run(dX, torch.empty_like(dX))
    Y = lower.solve(dX)
    F = ilu.factor()
    torch.cuda.synchronize()
    assert same_bits(B.values.cpu().numpy(), B2h.values)
    assert same_bits(P.cpu().numpy(), adv.ref_f64(B2h, X))
    assert same_bits(Y.cpu().numpy(), T.solve(B2h, X, True, False))
    assert same_bits(F.cpu().numpy(), reordered_factor("band2"))
    # an explicit permutation: no colours
    rev = np.arange(A.numRows)[::-1].copy()
    Re = dA.reordered(rev)
    assert Re.ncolors is None and Re.color is None
    Bev, vp = R.permute(A2, rev)
    torch.cuda.synchronize()
    assert np.array_equal(Re.vperm, vp) and same_bits(Re.B.values.cpu().numpy(), Bev.values)
    with pytest.raises(SmfvError, match="second time"):
        dA.reordered(np.zeros(A.numRows, np.int32))
    with pytest.raises(ValueError):
        dA.reordered("rcm")


@pytest.mark.parametrize("K,tiles", [(32, "force"), (3, "off")])
def test_order_keeping_identity(gpu, K, tiles):
    """spmm(ROWWISE, B, to_new(X)) == to_new(spmm(ROWWISE, A, X)) bit for bit,
    because a row of B keeps the CSR order of the row of A it came from: the
    square adversarial matrix (unsorted rows, repeated columns, special values
    in A and X), at K = 32 on a tiled plan and at K = 3 on the untiled row
    kernel."""
    pb = problem()
    dA, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    Rd = dA.reordered()
    pa = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles=tiles)
    pbb = smfv.SpmmPlan(smfv.Variant.ROWWISE, Rd.B, K, tiles=tiles)
    assert pa.stats()["tiled"] == pbb.stats()["tiled"] == (tiles == "force")
    YA = pa.run(dX, torch.empty_like(dX))
    YB = pbb.run(Rd.to_new(dX), torch.empty_like(dX))
    left, right = YB.cpu().numpy(), Rd.to_new(YA).cpu().numpy()
    assert adv.same(YA.cpu().numpy(), pb.Yref[:, :K])
    nan = np.isnan(right)
    assert np.array_equal(np.isnan(left), nan) and nan.any() and not nan.all()
    assert same_bits(left, right)
    assert same_bits(Rd.to_old(YB).cpu().numpy(), YA.cpu().numpy())
    # the library's spmm on the renumbered matrix through the cache
    assert same_bits(smfv.spmm(smfv.Variant.ROWWISE, Rd.B, Rd.to_new(dX)).cpu().numpy(), right)


# ---------------------------------------------------------------------------
# ILU(0) and the solves on B
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def reordered_factor(name):
    """ilu0_ref.factor of the host-renumbered matrix (band, band2, grid9)."""
    Bh, vperm = R.renumbered("band" if name == "band2" else name)
    if name == "band2":
        Bh = adv.Csr(np.asarray(I.band2().values)[vperm], Bh.colIndices, Bh.rowPtr, Bh.numRows, Bh.numCols)
    f = I._frozen(I.factor(Bh))
    assert np.isfinite(f).all()
    return f


@functools.lru_cache(None)
def reordered_applied(name, K=40):
    """(X, Z, Y): Z = U^-1 L^-1 (P X) by trsm_ref.solve applied twice to the
    reference factors of B, Y = P^T Z."""
    Bh, _ = R.renumbered("band" if name == "band2" else name)
    perm = R.ordering("band" if name == "band2" else name)[0]
    Fm = adv.Csr(reordered_factor(name), Bh.colIndices, Bh.rowPtr, Bh.numRows, Bh.numCols)
    X = I._frozen(np.random.default_rng(31).uniform(-1, 1, (Bh.numRows, K)))
    Z = I._frozen(T.solve(Fm, T.solve(Fm, X[perm], True, True), False, False))
    assert np.isfinite(Z).all()
    return X, Z, I._frozen(expected(REORDER_TO_OLD, perm, Z))


@pytest.mark.parametrize("K", [1, 32, 40])
@pytest.mark.parametrize("name", ["band", "grid9"])
def test_factor_and_solves_on_B(gpu, name, K):
    """ILU(0) of B, then both solves, against ilu0_ref and trsm_ref run on the
    host-renumbered matrix; the device plans have at most ncolors levels
    (`band`: 953 before); Ilu0Preconditioner(reorder="multicolor").apply(X)
    equals to_old of that reference applied to to_new(X)."""
    X, Z, Y = reordered_applied(name)
    nc = R.ordering(name)[2]
    dA = csr_of(R.INPUTS[name](), gpu)
    Rd = dA.reordered("multicolor")
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    F = smfv.ilu0(Rd.B)
    Zd = smfv.sptrsm(F, smfv.sptrsm(F, Rd.to_new(dX), "lower", True), "upper")
    torch.cuda.synchronize()
    assert same_bits(F.values.cpu().numpy(), reordered_factor(name))
    assert same_bits(Zd.cpu().numpy(), Z[:, :K])
    levels = (Rd.B.ilu0_plan().stats()["levels"], F.trsm_plan(K, "lower", True).stats()["levels"],
              F.trsm_plan(K, "upper").stats()["levels"])
    print("REORDER", name, "colours", nc, "levels ilu0 / lower / upper", levels)
    assert all(0 < l <= nc for l in levels)
    if name == "band":
        assert dA.ilu0_plan().stats()["levels"] == 953 and nc < 50
    M = smfv.Ilu0Preconditioner(dA, K, reorder="multicolor")
    assert M.R.ncolors == nc and M.plan.stats()["levels"] <= nc and M.lower.stats()["levels"] <= nc
    Yd = M.apply(dX)
    torch.cuda.synchronize()
    assert same_bits(Yd.cpu().numpy(), Y[:, :K])
    assert same_bits(dX.cpu().numpy(), X[:, :K]), "X changed"
    W = dX.clone()
    assert M.apply(W, W) is W  # the result may replace X: X is consumed by to_new first
    torch.cuda.synchronize()
    assert same_bits(W.cpu().numpy(), Y[:, :K])
    M2 = smfv.Ilu0Preconditioner(dA, K, reorder=Rd)  # a ReorderedCSR the caller already holds
    assert M2.R is Rd and same_bits(M2.apply(dX).cpu().numpy(), Y[:, :K])


def test_natural_order_unchanged(gpu):
    """reorder=None (the default) still gives the natural-order result, which
    differs from the multicolour one: another preconditioner."""
    K = 32
    X, Y = I.applied("band")
    dA = csr_of(I.band(), gpu)
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    for M in (smfv.Ilu0Preconditioner(dA, K), smfv.Ilu0Preconditioner(dA, K, reorder=None)):
        assert M.R is None and M.plan.stats()["levels"] == 953
        assert same_bits(M.apply(dX).cpu().numpy(), Y[:, :K])
    Xr, _, Yr = reordered_applied("band")
    assert np.array_equal(Xr, X) and not np.array_equal(Yr, Y)


def test_preconditioner_refactor(gpu):
    """refactor() after a value change refreshes B's values first: apply gives
    band2's multicolour result."""
    K = 32
    X, _, Y = reordered_applied("band")
    _, _, Y2 = reordered_applied("band2")
    assert not np.array_equal(Y, Y2)
    dA = csr_of(I.band(), gpu)
    dX = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    M = smfv.Ilu0Preconditioner(dA, K, reorder="multicolor")
    assert same_bits(M.apply(dX).cpu().numpy(), Y[:, :K])
    dA.values.copy_(torch.from_numpy(np.array(I.band2().values)))
    M.refactor()
    Z = M.apply(dX)
    torch.cuda.synchronize()
    assert same_bits(M.F.values.cpu().numpy(), reordered_factor("band2"))
    assert same_bits(Z.cpu().numpy(), Y2[:, :K])


# ---------------------------------------------------------------------------
# capture and streams
# ---------------------------------------------------------------------------
def _sequence(dA, K, gpu):
    """values, factor, both binds, to_new, both solves, to_old as one function of a stream."""
    M = smfv.Ilu0Preconditioner(dA, K, reorder="multicolor")
    dX = torch.full((dA.m, K), NAN, dtype=torch.float64, device=gpu)
    Yb = torch.full((dA.m, K), NAN, dtype=torch.float64, device=gpu)

    def steps(s):
        M.refactor(s)
        M.apply(dX, Yb, s)
    return M, dX, Yb, steps


def test_captured_sequence(gpu):
    """Captured once (global capture mode: a hidden allocation, synchronisation
    or null-stream launch is an error), replayed on another X and, after the
    values of A were overwritten with band2's, on other values."""
    K = 32
    X, _, Y = reordered_applied("band")
    _, _, Y2 = reordered_applied("band2")
    dA = csr_of(I.band(), gpu)
    M, dX, Yb, steps = _sequence(dA, K, gpu)
    torch.cuda.synchronize()
    M.F.values.fill_(NAN)
    M.R._B.values.fill_(NAN)
    g, side = capture(steps)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Yb).all()) and bool(torch.isnan(M.F.values).all()), "the capture executed"
    dX.copy_(torch.from_numpy(np.array(X[:, :K])))
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(Yb.cpu().numpy(), Y[:, :K])
    Xo = np.array(X[:, 8:8 + K])  # another X: the columns are independent
    dX.copy_(torch.from_numpy(Xo))
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(Yb.cpu().numpy(), Y[:, 8:8 + K])
    dA.values.copy_(torch.from_numpy(np.array(I.band2().values)))
    dX.copy_(torch.from_numpy(np.array(X[:, :K])))
    Yb.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(M.F.values.cpu().numpy(), reordered_factor("band2"))
    assert same_bits(Yb.cpu().numpy(), Y2[:, :K]), "the replay carries the values over, factors and binds again"
    del g


def test_stream_order(gpu):
    """The same sequence eagerly on a side stream with no device-wide sync."""
    K = 32
    X, _, _ = reordered_applied("band")
    _, _, Y2 = reordered_applied("band2")
    dA = csr_of(I.band(), gpu)
    M, dX, Yb, steps = _sequence(dA, K, gpu)
    dA.values.copy_(torch.from_numpy(np.array(I.band2().values)))
    Xsrc = torch.from_numpy(np.array(X[:, :K])).to(gpu)
    s = torch.cuda.Stream()
    Yout = in_stream_order(s, dX, Xsrc, steps, Yb, gpu)
    torch.cuda.synchronize()
    assert same_bits(Yout.cpu().numpy(), Y2[:, :K])


# ---------------------------------------------------------------------------
# refusals: nothing is launched and the output is untouched
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    m, K = 65, 32
    perm = np.random.default_rng(3).permutation(m).astype(np.int32)
    plan = RowsPlan(perm)
    X = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (m, K))).to(gpu)
    Y = torch.full((m, K), NAN, dtype=torch.float64, device=gpu)
    x, y = X.data_ptr(), Y.data_ptr()
    for args, word in (((REORDER_TO_NEW, x, K, K, x, K), "must not be X"), ((REORDER_TO_NEW, x, K, 0, y, K), "K = 0"),
                       ((REORDER_TO_OLD, x, K, -1, y, K), "K = -1"), ((REORDER_TO_NEW, None, K, K, y, K), "null"),
                       ((REORDER_TO_NEW, x, K, K, None, K), "null"), ((0, x, K, K, y, K), "direction"),
                       ((3, x, K, K, y, K), "direction"), ((8, x, K, K, y, K), "direction"),
                       ((REORDER_STORE_NT, x, K, K, y, K), "direction"), ((REORDER_TO_OLD, x, K - 1, K, y, K), "leading"),
                       ((REORDER_TO_NEW, x, K, K, y, K - 2), "leading")):
        assert plan.rows(*args) == -1 and word in lib.smfv_last_error().decode(), (args, lib.smfv_last_error())
    assert lib.smfv_reorder_plan_rows(None, REORDER_TO_NEW, x, K, K, y, K, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all()), "a refused call wrote Y"
    # values: in place and NULL are refused
    A = I.grid9()
    dA = csr_of(A, gpu)
    Rd = dA.reordered()
    v = dA.values.data_ptr()
    assert lib.smfv_reorder_plan_values(Rd._plan, v, v, None) == -1 and "in place" in lib.smfv_last_error().decode()
    assert lib.smfv_reorder_plan_values(Rd._plan, v, None, None) == -1
    with pytest.raises(ValueError):
        Rd.to_new(X)  # 65 rows, the matrix has 576
    with pytest.raises(TypeError):
        Rd.to_new(torch.zeros((A.numRows, 4), device=gpu))  # float32
    with pytest.raises(ValueError, match="square"):
        csr_of(adv.adv_pattern(300, 200, 2), gpu).reordered()
    with pytest.raises(ValueError, match="another matrix"):
        smfv.Ilu0Preconditioner(csr_of(A, gpu), 4, reorder=Rd)
    # the device is still usable
    assert plan.rows(REORDER_TO_NEW, x, K, K, y, K) == 0
    torch.cuda.synchronize()
    assert same_bits(Y.cpu().numpy(), X.cpu().numpy()[perm])
