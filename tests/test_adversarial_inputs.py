"""CPU checks of the adversarial inputs (tests/adversarial.py) that the GPU
parity tests of test_gpu_adversarial.py run: the oracle agrees with the
independent fp64 loop on them, the inputs hold the special classes they are
built for (so they cannot quietly turn benign), and the host plan analyses --
which replay the kernels' reads -- verify on the unsorted pattern with
repeats and on the degenerate shapes.  Recipe: m = n = 3000, seed 1, K = 8."""
import ctypes

import numpy as np
import pytest

import adversarial as adv
from oracle import oracle

from sparsematrixmultiplicationmpi_amd import _lib

M = N = 3000
SEED, K = 1, 8
LIVE, SINGLE_ROWS, ROW_PAIRS = 8192, 16384, 32768  # SMFV_PLAN_LIVE_VALUES / SINGLE_ROWS / ROW_PAIRS
ROW_FLAGS = (0, 1024, 2048, 4096, LIVE, ROW_PAIRS, LIVE | ROW_PAIRS, SINGLE_ROWS)
DEGENERATE = [(1, 500), (500, 1), (1, 1), (2000, 3)]
ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def problem():
    P = adv.adv_pattern(M, N, SEED, adv.LONG_ROWS)
    X = np.random.default_rng(SEED).uniform(-1, 1, (N, K))
    A, X, info = adv.adv_values(P, X)
    return A, X, info, adv.ref_f64(A, X)


def test_oracle_equals_independent_loop(problem):
    A, X, info, Yref = problem
    Yseq = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    assert adv.same(Yseq, Yref)
    for variant in ("rowwise", "columnwise"):
        for p in (1, 3):
            assert adv.same(oracle.spmm(variant, A.rowPtr, A.colIndices, A.values, X, p), Yseq), (variant, p)


def test_inputs_are_adversarial(problem):
    A, X, info, Yref = problem
    lens = np.diff(A.rowPtr)
    assert set(np.unique(lens % 8)) == set(range(8)) and (lens == 0).sum() > 50
    # unsorted rows, and repeats that are not adjacent
    unsorted = repeats = 0
    for r in range(M):
        c = A.colIndices[A.rowPtr[r]:A.rowPtr[r + 1]]
        unsorted += bool(np.any(np.diff(c) < 0))
        first = {}
        repeats += any(first.setdefault(int(v), i) < i - 1 for i, v in enumerate(c))
    assert unsorted > M // 2 and repeats > 200
    assert A.colIndices[A.rowPtr[adv.WIDE_ROW]:A.rowPtr[adv.WIDE_ROW + 1]].tolist() == [N - 1, 0, N - 1]
    assert all(lens[r] == L for r, L in adv.LONG_ROWS.items())
    va = A.values
    assert (va == 0).sum() > A.nnz // 10 and np.signbit(va[va == 0]).sum() > A.nnz // 20
    assert (np.abs(va) > 1e150).sum() > 100 and ((np.abs(va) < 1e-150) & (va != 0)).sum() > 100
    # the special classes in the reference result
    nan_rows = np.isnan(Yref).any(axis=1)
    inf_rows = np.isinf(Yref).any(axis=1)
    sub = (Yref != 0) & (np.abs(Yref) < np.finfo(np.float64).tiny)
    assert nan_rows.sum() >= 5 and inf_rows.sum() >= 5 and sub.sum() >= 5
    assert sub[info["subnormal_rows"]].all()
    # the cap that keeps the NONZERO comparison meaningful
    assert (~np.isfinite(Yref)).any(axis=1).sum() <= 0.05 * M
    # the constructed rows: every product -0.0, or exact cancellation; the sum is +0.0
    assert len(info["negzero_rows"]) >= 20 and len(info["cancel_rows"]) >= 20
    for r in info["negzero_rows"]:
        j = slice(A.rowPtr[r], A.rowPtr[r + 1])
        prod = va[j, None] * X[A.colIndices[j]]
        assert prod.size and np.all(prod == 0) and np.all(np.signbit(prod)), r
    assert np.all(lens[info["cancel_rows"]] >= 2)
    Z = Yref[info["zero_rows"]]
    assert np.all(Z == 0) and not np.signbit(Z).any()
    # finite_only keeps the zeros, subnormals and 2^+-600, drops what overflows or poisons
    P = adv.adv_pattern(M, N, SEED, adv.LONG_ROWS)
    Af, Xf, info_f = adv.adv_values(P, np.random.default_rng(SEED).uniform(-1, 1, (N, K)), finite_only=True)
    Yf = adv.ref_f64(Af, Xf)
    assert np.isfinite(Xf).all() and np.isfinite(Yf).all()
    poisoned = A.rowPtr[info["poison_rows"]]
    assert len(poisoned) >= 6 and not np.isfinite(va[poisoned]).any() and np.all(lens[info["poison_rows"] - 1] % 2 == 1)
    assert not np.isfinite(Yref[info["poison_rows"]]).any()
    keep = np.ones(A.nnz, bool)
    keep[poisoned] = False
    assert np.isfinite(va[keep]).all() and np.array_equal(adv.bits(Af.values)[keep], adv.bits(va)[keep])
    assert np.array_equal(info_f["zero_rows"], info["zero_rows"])
    assert np.signbit(Xf[info["x_special"]["-0"]]).all() and np.all(Xf[info["x_special"]["5e-324"]] == 5e-324)
    scale = adv.scale_hi(Af, Xf)
    assert np.all(scale < 1e300)


def _wrong_sum(A, X, mistake):
    """The reference loop with one plausible kernel mistake built in."""
    tiny = np.finfo(np.float64).tiny
    ftz = (lambda v: np.where(np.abs(v) < tiny, 0.0 * v, v)) if mistake == "flush" else (lambda v: v)
    Y = np.zeros((A.numRows, X.shape[1]))
    with np.errstate(all="ignore"):
        for r in range(A.numRows):
            j = np.arange(A.rowPtr[r], A.rowPtr[r + 1])
            c, a = A.colIndices[j], A.values[j]
            if mistake == "sorted":  # the row's entries in column order, not CSR order
                o = np.argsort(c, kind="stable")
                c, a = c[o], a[o]
            if mistake == "merged":  # a repeated column's values added up first
                c, inv = np.unique(c, return_inverse=True)
                a = np.bincount(inv, weights=a, minlength=c.size) if c.size else a
            s = np.zeros(X.shape[1])
            for i in range(c.size):
                p = ftz(a[i] * X[c[i]])
                s = p if (i == 0 and mistake == "first") else ftz(s + p)  # "first": no 0.0 + product
            Y[r] = s
    return Y


@pytest.mark.parametrize("mistake", ["first", "sorted", "merged", "flush"])
def test_inputs_tell_wrong_sums_apart(problem, mistake):
    """A sum that starts with its first product (-0.0 where the reference has
    +0.0), runs in column order, adds a repeated column's values first, or
    flushes subnormals differs from the reference under same() on these
    inputs -- on benign inputs (sorted unique columns, uniform values) the
    first three would not."""
    A, X, info, Yref = problem
    Y = _wrong_sum(A, X, mistake)
    assert not adv.same(Y, Yref)
    if mistake == "first":
        assert np.signbit(Y[info["negzero_rows"]]).all()
    if mistake == "flush":
        assert np.all(Y[info["subnormal_rows"]] == 0.0)


def _analyse_rows(A, r0, r1, flags):
    out = (ctypes.c_double * 9)()
    _lib.call("smfv_plan_analyse_rows", r0, r1, A.numCols, A.rowPtr.ctypes.data_as(ip), A.colIndices.ctypes.data_as(ip),
              flags, out)
    return {"tiles": int(out[0]), "direct": int(out[3]), "tiled_nnz": int(out[5])}


def _analyse_wsn(A, r0, r1, kw):
    out = (ctypes.c_double * 9)()
    _lib.call("smfv_wsn_plan_analyse", r0, r1, A.numCols, A.rowPtr.ctypes.data_as(ip), A.colIndices.ctypes.data_as(ip),
              kw, out)
    return {"tiles": int(out[0]), "direct": int(out[3]), "entries": int(out[5])}


def _analyse_chunks(A, r0, r1, cap=0):
    out = (ctypes.c_double * 6)()
    _lib.call("smfv_spmv_chunks_analyse", r0, r1, A.numCols, A.rowPtr.ctypes.data_as(ip),
              A.colIndices.ctypes.data_as(ip), cap, out)
    return {"fits": bool(out[0]), "chunks": int(out[1]), "entries": int(out[2]), "wide": bool(out[5])}


def test_host_plans_verify_on_the_pattern(problem):
    """The native build replays the kernel's reads of every plan it builds (a
    failed check fails the call): unsorted rows with non-adjacent repeats,
    the two long rows on the direct list."""
    A = problem[0]
    rp = A.rowPtr.astype(np.int64)
    for r0, r1 in ((0, M), (1001, 2500)):
        long_nnz = sum(L for r, L in adv.LONG_ROWS.items() if r0 <= r < r1)
        nnz = int(rp[r1] - rp[r0])
        for flags in ROW_FLAGS:
            a = _analyse_rows(A, r0, r1, flags)
            assert a["tiles"] >= 1 and a["tiled_nnz"] == nnz - long_nnz, (r0, r1, flags, a)
        for kw in (4, 8):
            w = _analyse_wsn(A, r0, r1, kw)
            assert w["tiles"] >= 1 and w["entries"] >= nnz - long_nnz, (r0, r1, kw, w)
    # K = 1 chunks: the 1,300-entry row does not fit the default 1,024-slot chunk
    assert not _analyse_chunks(A, 0, M)["fits"]
    B = adv.adv_pattern(M, N, SEED)
    for r0, r1 in ((0, M), (1001, 2500)):
        c = _analyse_chunks(B, r0, r1)
        assert c["fits"] and c["chunks"] >= 1 and not c["wide"] and c["entries"] == int(B.rowPtr[r1] - B.rowPtr[r0])
    # the row [n-1, 0, n-1] of an 80,000-column variant spans more than 2^16 columns: 32-bit columns
    W = adv.adv_pattern(M, 80000, SEED)
    c = _analyse_chunks(W, 0, M)
    assert c["fits"] and c["wide"] and c["entries"] == W.nnz


@pytest.mark.parametrize("m,n", DEGENERATE)
def test_host_plans_verify_on_degenerate_shapes(m, n):
    A = adv.adv_degenerate(m, n, SEED)
    assert A.nnz >= 1
    for flags in ROW_FLAGS:  # (the 300-entry row is over geometry 2's tile: a direct row there)
        a = _analyse_rows(A, 0, m, flags)
        assert (a["tiles"] >= 1 and a["tiled_nnz"] == A.nnz) or (m == 1 and a["direct"] == 1), (flags, a)
    for kw in (4, 8):
        w = _analyse_wsn(A, 0, m, kw)
        assert w["tiles"] >= 1 and w["direct"] == 0 and w["entries"] >= A.nnz, (kw, w)
    c = _analyse_chunks(A, 0, m)
    assert c["fits"] and c["entries"] == A.nnz


@pytest.mark.parametrize("kind", ["long", "short"])
def test_large_offset_conditions(kind):
    """What test_gpu_large_offsets.py rests on, without a GPU: each leading
    dimension's span n * ld * 8 lies on the stated side of 2^31 / 2^32, and on
    the patterns that file runs at least a quarter of the entries read X at a
    byte offset >= 2^31 at ld C and >= 2^32 at ld E (uniform columns give a
    half and a third)."""
    A = adv.adv_pattern(M, N, SEED, adv.LONG_ROWS if kind == "long" else None)
    share_c, share_e = adv.large_offset_conditions(A)
    print("entry shares: >= 2^31 at C", share_c, ">= 2^32 at E", share_e)
    assert 0.4 < share_c < 0.6 and 0.25 < share_e < 0.45
    # the row block [1001, 2500) reads beyond 2^32 at E as well
    s, e = int(A.rowPtr[1001]), int(A.rowPtr[2500])
    assert np.mean(A.colIndices[s:e].astype(np.int64) * adv.LARGE_LD["E"] * 8 >= 1 << 32) >= 0.25
