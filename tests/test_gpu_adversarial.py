"""Every kernel path on adversarial inputs (tests/adversarial.py): unsorted
rows with non-adjacent repeated columns, signed zeros, subnormals, 2^+-600,
+-inf, NaN and +-1.7e308 in A and in X, rows whose reference sum is exactly
+0.0, misaligned X / Y views and degenerate shapes.

Bit-exact paths are compared with adversarial.ref_f64 -- a plain numpy loop in
CSR order that shares no code with oracle/ (the oracle itself is checked
against it in test_adversarial_inputs.py) -- under adversarial.same(): NaN
exactly where the reference has NaN, identical bits elsewhere, the sign of
zero and of inf included.  The reassociating paths (NONZERO on the merge
path, the FMA and MFMA opt-ins) are held to the project's own tolerance,
1e-12 x sum|a||x| + 1e-300 (test_gpu_parity.py), against the np.longdouble
loop; the opt-ins on the finite input (the MFMA plan requires a finite X:
include/smfv.h).  m = n = 3000: several tiles per XCD, two direct rows,
several K = 1 chunks.
"""
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
from test_gpu_dist_parity import assemble, replay_exchange

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import dist as D

pytestmark = pytest.mark.gpu
M = N = 3000
SEED = 1
V = smfv.Variant
BITWISE = (V.SEQUENTIAL, V.ROWWISE, V.COLUMNWISE)
ROWS = (1001, 2500)


class Problem:
    """One adversarial (A, X) with its references, computed once and read-only."""

    def __init__(self, A, X, info):
        self.A, self.X, self.info = A, X, info
        self._dev = None

    @functools.cached_property
    def Yref(self):
        return _frozen(adv.ref_f64(self.A, self.X))

    @functools.cached_property
    def Yhi(self):
        return _frozen(adv.ref_hi(self.A, self.X))

    @functools.cached_property
    def scale(self):
        return _frozen(adv.scale_hi(self.A, self.X))

    def dev(self, gpu):
        if self._dev is None:
            A = self.A
            dA = smfv.DeviceCSR(smfv.SparseMatrix(A.values, A.colIndices, A.rowPtr, A.numRows, A.numCols), gpu)
            self._dev = (dA, torch.from_numpy(self.X).to(gpu))
        return self._dev


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def problem(kind="long", finite=False, kx=128):
    """kind: "long" (rows 100 and 2000 of 700 / 1,300 entries: direct rows),
    "short" (no row over 1,024: the K = 1 chunk layout fits), "wide" (short,
    n = 80,000: the row [n-1, 0, n-1] spans more than 2^16 columns)."""
    n = 80000 if kind == "wide" else N
    P = adv.adv_pattern(M, n, SEED, adv.LONG_ROWS if kind == "long" else None)
    X = np.random.default_rng(SEED).uniform(-1, 1, (n, kx))
    return Problem(*adv.adv_values(P, X, finite_only=finite))


def execute(plan, Xv, m_out, K, gpu, g=0, pad=2):
    """Run into the window [g, g + K) of a NaN-filled (K + g + pad)-wide
    buffer; the columns on both sides of the window must stay NaN."""
    Yb = torch.full((m_out, g + K + pad), np.nan, dtype=torch.float64, device=gpu)
    plan.run(Xv, Yb[:, g:g + K])
    torch.cuda.synchronize()
    Yh = Yb.cpu().numpy()
    assert np.isnan(Yh[:, :g]).all() and np.isnan(Yh[:, g + K:]).all(), "Y written outside its window"
    return np.ascontiguousarray(Yh[:, g:g + K])


def note(case, st):
    """The path a case ran, as stats() tells it (shown with pytest -s / -rP)."""
    keys = ("tiled", "kernel", "ws_geom", "live_values", "paired_rows", "direct_rows", "tiles", "mfma")
    print("PATH", case, {k: st[k] for k in keys if k in st})


def check_tol(Y, pb, cols, rows=slice(None)):
    ok, worst = adv.within_tol(Y, pb.Yhi[rows, cols], pb.scale[rows, cols], pb.Yref[rows, cols])
    print("TOL worst error / bound", worst)
    return ok


# ---------------------------------------------------------------------------
# untiled row kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 33, 2, 4, 8, 16, 32, 128])
def test_untiled_row_kernels(gpu, K):
    """k_rows (odd K) and every row_cfg_for class of k_rows_mh (tiles="off",
    aligned, range-checked X buffer) on the full special-value input."""
    pb = problem()
    dA, dX = pb.dev(gpu)
    for v in BITWISE:
        plan = smfv.SpmmPlan(v, dA, K, tiles="off")
        st = plan.stats()
        assert not st["tiled"], st
        note(f"untiled K={K} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :K], M, K, gpu), pb.Yref[:, :K]), (K, v)


@pytest.mark.parametrize("kind", ["long", "short", "wide"])
def test_spmv_k1(gpu, kind):
    """K = 1: k_spmv_stream (a 1,300-entry row keeps the pattern off the chunk
    layout), k_spmv_chunks with 16-bit offsets from the unsorted rows'
    minimum, and with 32-bit columns (a row spanning more than 2^16)."""
    pb = problem(kind, kx=1) if kind == "wide" else problem(kind)
    dA, dX = pb.dev(gpu)
    for v in BITWISE:
        plan = smfv.SpmmPlan(v, dA, 1)
        st = plan.stats()
        assert st["kernel"] == (None if kind == "long" else "k_spmv_chunks") and st["tiled"] == (kind != "long"), st
        note(f"k1 {kind} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :1], M, 1, gpu), pb.Yref[:, :1]), (kind, v)
        assert adv.same(execute(plan, dX[:, :1], M, 1, gpu, pad=0), pb.Yref[:, :1]), (kind, v)


# ---------------------------------------------------------------------------
# tiled kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("pairs", ["on", "off"])
@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("tk", ["ws1", "ws2", "ws3"])
def test_ws_tiles(gpu, tk, live, pairs, K):
    """k_rows_ws geometries 1 / 2 / 3, snapshot and live values, row pairs on
    and off, with the two long rows on k_rows_list: -0.0 pads against the
    zero image row, the live plans' read past odd rows, a first product of
    -0.0."""
    pb = problem()
    dA, dX = pb.dev(gpu)
    for v in V:
        plan = smfv.SpmmPlan(v, dA, K, tiles="force", tiled_kernel=tk, live_values=live, row_pairs=pairs)
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["ws_geom"] == int(tk[-1]), st
        assert st["live_values"] == live and (st["paired_rows"] > 0) == (pairs == "on"), st
        assert st["direct_rows"] >= 1, st
        note(f"ws {tk} live={live} pairs={pairs} K={K} {v.name}", st)
        assert adv.same(execute(plan, dX[:, :K], M, K, gpu), pb.Yref[:, :K]), (v, st)


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("tk", ["ws1", "ws2", "ws3"])
def test_ws_narrow_window(gpu, tk, live):
    """k_rows_ws NARROW: the 16-column window [16, 32) of a 32-wide X."""
    K, f = 16, 16
    pb = problem()
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :32].contiguous()
    for v in BITWISE:
        plan = smfv.SpmmPlan(v, dA, K, tiles="force", tiled_kernel=tk, live_values=live)
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["ws_geom"] == int(tk[-1]), st
        assert st["live_values"] == live and st["direct_rows"] >= 1, st
        note(f"ws narrow {tk} live={live} {v.name}", st)
        assert adv.same(execute(plan, dX32[:, f:f + K], M, K, gpu), pb.Yref[:, f:f + K]), (v, st)


@pytest.mark.parametrize("K", [4, 8])
def test_wsn_tiles(gpu, K):
    """k_rows_wsn: the window of 4 / 8 columns of a 32-wide X."""
    f = 32 - K - 4
    pb = problem()
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :32].contiguous()
    for v in BITWISE:
        plan = smfv.SpmmPlan(v, dA, K, tiles="force")
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_wsn" and st["direct_rows"] >= 1, st
        note(f"wsn K={K} {v.name}", st)
        assert adv.same(execute(plan, dX32[:, f:f + K], M, K, gpu), pb.Yref[:, f:f + K]), (v, st)


@pytest.mark.parametrize("K,kind", [(32, "long"), (1, "long"), (1, "short")])
def test_row_block_plans(gpu, K, kind):
    """Plans of the row block [1001, 2500): forced tiles (snapshot and live,
    one direct row) at K = 32; k_spmv_stream and k_spmv_chunks at K = 1."""
    pb = problem(kind)
    dA, dX = pb.dev(gpu)
    r0, r1 = ROWS
    for v in BITWISE:
        for live in ((False, True) if K == 32 else (False,)):
            plan = smfv.SpmmPlan(v, dA, K, tiles="force", rows=ROWS, live_values=live)
            st = plan.stats()
            if K == 32:
                assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["row_begin"] == r0, st
                assert st["direct_rows"] >= 1 and st["live_values"] == live, st
            else:
                assert st["kernel"] == (None if kind == "long" else "k_spmv_chunks"), st
            note(f"rows{ROWS} K={K} {kind} live={live} {v.name}", st)
            assert adv.same(execute(plan, dX[:, :K], r1 - r0, K, gpu), pb.Yref[r0:r1, :K]), (v, st)


# ---------------------------------------------------------------------------
# the reassociating paths: NONZERO on the merge path, FMA, MFMA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 8, 33])
def test_merge_path(gpu, K):
    """NONZERO with tiles="off": k_merge_flat (K = 32), k_merge + k_carry_fixup
    (K = 8 vectorised, K = 33 scalar) on the full special-value input: within
    the tolerance where the scale is finite, non-finite wherever the reference
    is elsewhere, the same bits on a second run."""
    pb = problem()
    dA, dX = pb.dev(gpu)
    plan = smfv.SpmmPlan(V.NONZERO, dA, K, tiles="off")
    st = plan.stats()
    assert not st["tiled"], st
    note(f"merge K={K}", st)
    Y = execute(plan, dX[:, :K], M, K, gpu)
    assert check_tol(Y, pb, slice(0, K))
    assert np.array_equal(adv.bits(execute(plan, dX[:, :K], M, K, gpu)), adv.bits(Y))


@pytest.mark.parametrize("K", [32, 16, 8])
def test_fma_opt_in(gpu, K):
    """SMFV_PLAN_FMA on the finite input (k_rows_ws, its NARROW form,
    k_rows_wsn): within the tolerance, and the constructed rows -- every
    product -0.0, or a*x then (-a)*x with exact products -- still +0.0."""
    pb = problem(finite=True)
    dA, dX = pb.dev(gpu)
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", fma=True)
    st = plan.stats()
    assert st["tiled"] and st["kernel"] == ("k_rows_wsn" if K == 8 else "k_rows_ws"), st
    note(f"fma K={K}", st)
    Y = execute(plan, dX[:, :K], M, K, gpu)
    assert check_tol(Y, pb, slice(0, K))
    Z = Y[pb.info["zero_rows"]]
    assert np.all(Z == 0.0) and not np.signbit(Z).any()


def test_mfma_opt_in(gpu):
    """SMFV_PLAN_MFMA on the finite input (its contract: the dense blocks'
    zeros multiply every staged X row, so an inf or NaN in X would reach rows
    that do not reference it): within the tolerance."""
    K = 32
    pb = problem(finite=True)
    dA, dX = pb.dev(gpu)
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", mfma=True)
    st = plan.stats()
    assert st["mfma"] and st["kernel"] == "k_rows_mfma", st
    note("mfma K=32", st)
    assert check_tol(execute(plan, dX[:, :K], M, K, gpu), pb, slice(0, K))


# ---------------------------------------------------------------------------
# rank plans
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [V.ROWWISE, V.COLUMNWISE, V.NONZERO])
def test_rank_plans(gpu, variant):
    """Every rank's plan at p = 3 (smfv_dist_plan_create_rank, forced tiles)
    and the native exchange schedule replayed on the device, as
    test_gpu_dist_parity.test_rank_plans_vs_reference does it: ROWWISE and
    COLUMNWISE bit for bit, NONZERO (rows cut between ranks) in tolerance."""
    K, p = 32, 3
    pb = problem()
    A = pb.A
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :K].contiguous()
    root = p - 1
    first, last, off, cnt = D.exchange_plan(variant, M, A.nnz, A.rowPtr, K, p, D.dist_opts("reference"))
    Y = torch.full((M, K), float("nan"), dtype=torch.float64, device=gpu)
    blocks, plans = [], []
    for r in range(p):
        P = D.DistPlan(None, variant, dA, K, to_all=False, root=root, tiles="force", rank=(r, p))
        plans.append(P)
        P.run_local(dX32, Y)
        blocks.append(P.exchange_buffer())
        if variant == V.ROWWISE:
            assert P.stats()["tiled"], P.stats()
        print("PATH rank plan", variant.name, r, P.stats())
    if variant != V.ROWWISE:
        xbuf = torch.full((max(int((off + cnt).max()), 1),), float("nan"), dtype=torch.float64, device=gpu)
        replay_exchange(variant, A, K, p, root, blocks, xbuf)
        Y.fill_(float("nan"))
        assemble(variant, A, K, p, xbuf, Y, first, last)
    torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    if variant == V.NONZERO:
        assert check_tol(Yh, pb, slice(0, K))
    else:
        assert adv.same(Yh, pb.Yref[:, :K])


# ---------------------------------------------------------------------------
# misaligned views
# ---------------------------------------------------------------------------
VIEWS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (0, 0)]


@pytest.mark.parametrize("K", [32, 8, 1])
def test_misaligned_views(gpu, K):
    """X windows [f, f + K) of a 40-wide buffer into Y windows [g, g + K) of a
    (K + 4)-wide one: even strides on 8- or 16-byte bases.  One plan object
    per variant (forced tiles; a live-values plan; at K = 1 the chunk plan)
    runs all the views in turn and the first again: the kernel is picked at
    every execute (pick_vec) -- the tiled one on 16-byte bases, k_rows / the
    merge path on 8-byte ones."""
    pb = problem("short" if K == 1 else "long", finite=True, kx=40)
    dA, dX = pb.dev(gpu)
    plans = [(v, smfv.SpmmPlan(v, dA, K, tiles="force")) for v in V]
    plans.append((V.ROWWISE, smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", live_values=True)))
    for v, plan in plans:
        st = plan.stats()
        # (a live plan of an 8-column window is k_rows_ws NARROW; a K = 1 plan keeps its snapshot)
        want = {32: "k_rows_ws", 8: "k_rows_ws" if st["live_values"] else "k_rows_wsn", 1: "k_spmv_chunks"}[K]
        assert st["tiled"] and st["kernel"] == want, st
        note(f"views K={K} {v.name} live={st['live_values']}", st)
    assert plans[-1][1].stats()["live_values"] == (K != 1)
    for f, g in VIEWS:
        cols = slice(f, f + K)
        for v, plan in plans:
            Y = execute(plan, dX[:, cols], M, K, gpu, g=g, pad=4 - g)
            if v == V.NONZERO:
                assert check_tol(Y, pb, cols), (f, g)
            else:
                assert adv.same(Y, pb.Yref[:, cols]), (f, g, v, plan.stats()["live_values"])


# ---------------------------------------------------------------------------
# degenerate shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 500), (500, 1), (1, 1), (2000, 3)])
def test_degenerate_shapes(gpu, m, n):
    """One 300-entry row, one column, one entry, three columns -- random
    columns, hence repeats -- at K = 1 / 4 / 8 / 32, forced and automatic
    plans, every variant: bit-identical to the fp64 loop (a NONZERO plan that
    stats() shows on the merge path: within the tolerance)."""
    A = adv.adv_degenerate(m, n, SEED)
    X = np.random.default_rng(SEED).uniform(-1, 1, (n, 32))
    if n >= 3:
        X[-1] = -0.0
    pb = Problem(A, X, None)
    dA, dX = pb.dev(gpu)
    for K in (1, 4, 8, 32):
        for tiles in ("force", "auto"):
            for v in V:
                plan = smfv.SpmmPlan(v, dA, K, tiles=tiles)
                st = plan.stats()
                note(f"degenerate {m}x{n} K={K} {tiles} {v.name}", st)
                Y = execute(plan, dX[:, :K], m, K, gpu)
                if v == V.NONZERO and not st["tiled"]:
                    assert check_tol(Y, pb, slice(0, K)), (K, tiles)
                else:
                    assert adv.same(Y, pb.Yref[:, :K]), (K, tiles, v, st)


# ---------------------------------------------------------------------------
# the device compare (smfvCompareWithReference)
# ---------------------------------------------------------------------------
def _np_compare(a, b):
    d = np.abs(a - b)
    return float(d.max()), float((d / np.maximum(np.abs(b), 1e-300)).max())


def test_compare_relative_figure(gpu):
    """The largest absolute and the largest relative difference sit at
    different elements; both figures equal numpy's."""
    a = np.random.default_rng(3).uniform(1, 2, (300, 7))
    b = a.copy()
    a[17, 3], b[17, 3] = 100.0, 100.5
    a[5, 2], b[5, 2] = 0.5, 0.25
    mabs, mrel = smfv.compare(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu))
    assert (mabs, mrel) == _np_compare(a, b) and mabs == 0.5 and mrel == 1.0


def test_compare_far_element(gpu):
    """More elements than the grid-stride loop's 1024 x 256 lanes, the total
    no multiple of 256: a single difference in the last element is found."""
    m, K = 1200, 257
    assert m * K > 1024 * 256 and (m * K) % 256
    a = torch.from_numpy(np.random.default_rng(4).uniform(1, 2, (m, K))).to(gpu)
    b = a.clone()
    assert smfv.compare(a, b) == (0.0, 0.0)
    b[m - 1, K - 1] += 0.25
    assert smfv.compare(a, b) == _np_compare(a.cpu().numpy(), b.cpu().numpy())
    assert smfv.compare(a, b)[0] == 0.25


def test_compare_nan_policy_and_views(gpu):
    """A NaN in A alone, or in A and B at the same element, is a difference
    (inf for both figures: the policy test_host.py documents); NaN in the
    padding of views with lda / ldb > K is not read; an empty pair is (0, 0)."""
    a = torch.from_numpy(np.random.default_rng(5).uniform(1, 2, (300, 7))).to(gpu)
    b = a.clone()
    an = a.clone()
    an[123, 4] = float("nan")
    assert smfv.compare(an, b) == (float("inf"), float("inf"))
    assert smfv.compare(an, an.clone()) == (float("inf"), float("inf"))
    Ab = torch.full((300, 10), float("nan"), dtype=torch.float64, device=gpu)
    Bb = torch.full((300, 12), float("nan"), dtype=torch.float64, device=gpu)
    Ab[:, :7], Bb[:, 2:9] = a, b
    assert smfv.compare(Ab[:, :7], Bb[:, 2:9]) == (0.0, 0.0)
    Bb[299, 8] += 0.125
    assert smfv.compare(Ab[:, :7], Bb[:, 2:9])[0] == 0.125
    e = torch.empty((5, 0), dtype=torch.float64, device=gpu)
    assert smfv.compare(e, e.clone()) == (0.0, 0.0)
