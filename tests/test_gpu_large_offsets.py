"""Every kernel path reading X, and writing Y, beyond the 2 GiB and 4 GiB
byte offsets.

Several kernels pick between a 32-bit-offset form and a 64-bit-pointer form
of their X addressing at execute, from n * ldx * 8 (smfv_kernels.hip):
k_rows_mh's buffer loads up to 2^31 - 1 (launch_rows_mh: `buf = xb > 0 && xb
<= 0x7fffffffLL`), k_rows_ws's scalar-base DMAs below 2^32 (plan_launch:
`saddr = n * ldx * 8 < (1ull << 32) && ...`); the live-values and k_rows_wsn
tiles are 32-bit only and fall back to launch_rows from 2^32 on.  Y is
addressed as Y + (int64_t)row * ldy everywhere.

The problem stays the adversarial 3,000 x 3,000 one of test_gpu_adversarial.py;
the offsets come from the leading dimension.  One flat device buffer of
3,000 * LD_E doubles (6.4 GB) is refilled with NaN by every case and viewed as
(3000, ld)[:, f:f + K]: with the strides of adversarial.LARGE_LD the span
n * ld * 8 is just under 2^31 (A), just over it (B), just under 2^32 (C), just
over it (D: the dispatch flips, no offset reaches 2^32 yet) and 6 GiB (E:
columns >= 2,000 lie beyond 2^32).  A wrong address that stays inside the
allocation reads NaN or another row and fails the comparison.  The Y-wide
cases view the same buffer as Y with ldy = LD_E and a small contiguous X;
afterwards every element outside the window must still be NaN.

References as in test_gpu_adversarial.py: adversarial.ref_f64 under
adversarial.same() (bit for bit) for SEQUENTIAL / ROWWISE plans, the fused
epilogue as numpy's `alpha * S + beta * Y0` (test_gpu_axpby.py); the
reassociating paths (NONZERO on the merge path, FMA, MFMA) within 1e-12 x
sum|a||x| + 1e-300 of the np.longdouble loop (check_tol), FMA and MFMA on the
finite input.  The conditions all this rests on (span sides, the share of
entries beyond 2^31 at C and 2^32 at E) are asserted before the buffer is
allocated and, without a GPU, in test_adversarial_inputs.py.

Which instance an execute launched is not observable; each case asserts the
plan it built through stats() / epilogue_mode and names the instance that
follows from the dispatch.

Out of scope: a snapshot or CSR values array of 4 GiB or more (nnz >= 2^29),
and distributed plans (they take a contiguous X only).  X and Y element
offsets of 2^31 doubles or more (16 GiB) are not reached either: the largest
here is 3,000 * LD_E = 8.1e8.
"""
import functools

import numpy as np
import pytest
import torch

import adversarial as adv
from test_gpu_adversarial import check_tol, execute, note, problem
from test_gpu_axpby import ALPHA, BETA, expected

import sparsematrixmultiplicationmpi_amd as smfv

pytestmark = pytest.mark.gpu
M = N = adv.LARGE_N
LD = adv.LARGE_LD
LD_E = LD["E"]
V = smfv.Variant
ROWS = (1001, 2500)
F, G = 6, 10  # first column of the X / Y window: even, so rows stay 16-byte aligned
NAN = float("nan")
LONG = sorted(adv.LONG_ROWS)
GEOMS = ["ws1", "ws2", "ws3"]


def big():
    """The full special-value problem with 200 columns of X (K = 200 needs them)."""
    return problem(kx=200)


@functools.lru_cache(maxsize=None)
def y0():
    a = np.random.default_rng(7).uniform(-1, 1, (M, 200))
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def flat(gpu):
    for kind in ("long", "short"):
        adv.large_offset_conditions(problem(kind).A)
    assert problem().A.numCols == N and F % 2 == 0 and G % 2 == 0
    buf = torch.empty(M * LD_E, dtype=torch.float64, device=gpu)
    yield buf
    del buf
    torch.cuda.empty_cache()


def x_window(flat, ld, K, dX):
    """The buffer refilled with NaN, X[:, :K] in the window [F, F + K) of its (N, ld) view."""
    flat.fill_(NAN)
    Xv = flat[:N * ld].view(N, ld)[:, F:F + K]
    Xv.copy_(dX[:, :K])
    assert Xv.stride() == (ld, 1) and Xv.data_ptr() == flat.data_ptr() + 8 * F
    return Xv


def run_fused(plan, Xv, Y0, gpu):
    """run_axpby on a copy of Y0 in the first K columns of a (K + 2)-wide NaN buffer."""
    m, K = Y0.shape
    Yb = torch.full((m, K + 2), NAN, dtype=torch.float64, device=gpu)
    Yb[:, :K] = torch.tensor(Y0)
    plan.run_axpby(Xv, Yb[:, :K], ALPHA, BETA)
    torch.cuda.synchronize()
    Yh = Yb.cpu().numpy()
    assert np.isnan(Yh[:, K:]).all(), "padding of Y written"
    return np.ascontiguousarray(Yh[:, :K])


def both(gpu, Xv, pb, K, variant=V.ROWWISE, want=None, **kw):
    """A plain plan's run and a fused plan's run_axpby on the same X view, each
    bit for bit; `want` checks stats()."""
    dA, _ = pb.dev(gpu)
    S, Y0 = pb.Yref[:, :K], y0()[:, :K]
    plan = smfv.SpmmPlan(variant, dA, K, **kw)
    st = plan.stats()
    want(st)
    note(f"K={K} ldx={Xv.stride(0)} {variant.name} {kw}", st)
    Y = execute(plan, Xv, M, K, gpu)
    assert adv.same(Y[LONG], S[LONG]), ("rows 100 / 2000", st)
    assert adv.same(Y, S), ("plain", variant, st)
    fused = smfv.SpmmPlan(variant, dA, K, axpby=True, **kw)
    assert fused.epilogue_mode == "fused", (fused.epilogue_mode, fused.stats())
    want(fused.stats())
    assert adv.same(run_fused(fused, Xv, Y0, gpu), expected(S, Y0)), ("fused", variant, st)


def untiled(st):
    assert not st["tiled"], st


# ---------------------------------------------------------------------------
# 1, 2: the untiled row kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("span", ["A", "B", "E"])
@pytest.mark.parametrize("K", [2, 4, 8, 16, 32, 128, 6, 20, 100, 200])
def test_rows_mh(gpu, flat, K, span):
    """k_rows_mh, every row_cfg_for class (K = 2 ... 128) and K whose last
    column pass is partial, plain and Axpby.  launch_rows_mh: `buf = xb > 0 &&
    xb <= 0x7fffffffLL` -- span A runs BUF = true with offsets up to 2^31 - 1
    - 11,647; B and E run BUF = false (E: 64-bit offsets beyond 2^32)."""
    pb = big()
    Xv = x_window(flat, LD[span], K, pb.dev(gpu)[1])
    assert (N * LD[span] * 8 <= 0x7fffffff) == (span == "A")
    for v in (V.ROWWISE, V.SEQUENTIAL):
        both(gpu, Xv, pb, K, variant=v, want=untiled, tiles="off")


@pytest.mark.parametrize("K,ld", [(3, LD_E), (33, LD_E), (32, LD_E - 1)])
def test_rows_simple(gpu, flat, K, ld):
    """k_rows (launch_rows: pick_vec != 2): odd K at E, and an even K on the
    odd leading dimension E - 1; X + (int64_t)cc * ldx beyond 2^32."""
    pb = big()
    Xv = x_window(flat, ld, K, pb.dev(gpu)[1])
    assert K % 2 or ld % 2
    both(gpu, Xv, pb, K, want=untiled, tiles="off")


# ---------------------------------------------------------------------------
# 3: k_rows_ws on its snapshot
# ---------------------------------------------------------------------------
def ws(tk, live=False, pairs=None):
    def want(st):
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["ws_geom"] == int(tk[-1]), st
        assert st["live_values"] == live and st["direct_rows"] >= 1, st
        assert pairs is None or (st["paired_rows"] > 0) == pairs, st
    return want


@pytest.mark.parametrize("span", ["C", "D", "E"])
@pytest.mark.parametrize("K", [32, 64, 16])
@pytest.mark.parametrize("tk", GEOMS)
def test_ws_snapshot(gpu, flat, tk, K, span):
    """k_rows_ws / k_ws_axpby, geometries 1 / 2 / 3, one and two panels and the
    NARROW window (K = 16).  plan_launch: `saddr = n * ldx * 8 < (1ull << 32)`
    -- C runs the SADDR instances with `xo = uc * ldxb` up to 2^32 - 23,296; D
    and E the dma16 instances on 64-bit addresses.  Rows 100 and 2000 run in
    k_rows_list (k_rows_list_axpby), wide and narrow."""
    pb = big()
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD[span], K, dX)
    assert (N * LD[span] * 8 < 1 << 32) == (span == "C")
    if K == 64:  # (a fused K = 64 adds no instance: the panels share one)
        plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", tiled_kernel=tk)
        ws(tk)(plan.stats())
        note(f"ws {tk} K={K} {span}", plan.stats())
        assert adv.same(execute(plan, Xv, M, K, gpu), pb.Yref[:, :K])
    else:
        both(gpu, Xv, pb, K, want=ws(tk), tiles="force", tiled_kernel=tk)


@pytest.mark.parametrize("tk", GEOMS)
def test_ws_row_pairs(gpu, flat, tk):
    """Row pairs on, at E (the non-SADDR instance)."""
    pb = big()
    Xv = x_window(flat, LD_E, 32, pb.dev(gpu)[1])
    both(gpu, Xv, pb, 32, want=ws(tk, pairs=True), tiles="force", tiled_kernel=tk, row_pairs="on")


@pytest.mark.parametrize("span", ["C", "E"])
@pytest.mark.parametrize("K", [32, 16])
@pytest.mark.parametrize("tk", GEOMS)
def test_ws_fma(gpu, flat, tk, K, span):
    """The FMA instances (SADDR at C, dma16 at E) on the finite input, within the tolerance."""
    pb = problem(finite=True)
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD[span], K, dX)
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", tiled_kernel=tk, fma=True)
    ws(tk)(plan.stats())
    note(f"fma {tk} K={K} {span}", plan.stats())
    assert check_tol(execute(plan, Xv, M, K, gpu), pb, slice(0, K))


# ---------------------------------------------------------------------------
# 4, 5: the 32-bit-only tiles and their fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("span", ["C", "D", "E"])
@pytest.mark.parametrize("K", [32, 16])
@pytest.mark.parametrize("tk", GEOMS)
def test_live_values(gpu, flat, tk, K, span):
    """Live-values plans.  plan_launch: `if (!saddr || nnz * 8 >= (1ull <<
    32)) return launch_rows(..., ep)` -- at C k_rows_ws_live / k_ws_axpby_live
    run tiled with 32-bit offsets up to 2^32 - 23,296; at D and E the plan
    runs k_rows_mh<.., false> (and its Axpby instance: the fallback carries the
    epilogue)."""
    pb = big()
    Xv = x_window(flat, LD[span], K, pb.dev(gpu)[1])
    both(gpu, Xv, pb, K, want=ws(tk, live=True), tiles="force", tiled_kernel=tk, live_values=True)


@pytest.mark.parametrize("span", ["C", "D", "E"])
@pytest.mark.parametrize("K", [4, 8])
def test_wsn(gpu, flat, K, span):
    """k_rows_wsn (plan_launch: `if (n * ldx * 8 >= (1ull << 32) || ...)
    return launch_rows(...)`): tiled at C, k_rows_mh<.., false> at D and E; at
    E the two-pass axpby as well."""
    pb = big()
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD[span], K, dX)
    S = pb.Yref[:, :K]
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force")
    st = plan.stats()
    assert st["tiled"] and st["kernel"] == "k_rows_wsn" and st["direct_rows"] >= 1, st
    note(f"wsn K={K} {span}", st)
    assert adv.same(execute(plan, Xv, M, K, gpu), S), st
    if span == "E":
        two = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", axpby=True)
        assert two.epilogue_mode == "two_pass" and two.stats()["kernel"] == "k_rows_wsn", two.stats()
        Y0 = y0()[:, :K]
        assert adv.same(run_fused(two, Xv, Y0, gpu), expected(S, Y0))


# ---------------------------------------------------------------------------
# 6: K = 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["short", "long"])
def test_spmv_k1(gpu, flat, kind):
    """k_spmv_chunks ("short": `xb[j0 * ldx]` with 64-bit j0) and
    k_spmv_stream ("long": `X[(int64_t)c[i] * ldx]`) on one column at E."""
    pb = problem(kind)
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD_E, 1, dX)
    for v in (V.ROWWISE, V.SEQUENTIAL):
        plan = smfv.SpmmPlan(v, dA, 1)
        st = plan.stats()
        assert st["kernel"] == (None if kind == "long" else "k_spmv_chunks") and st["tiled"] == (kind != "long"), st
        note(f"k1 {kind} {v.name}", st)
        assert adv.same(execute(plan, Xv, M, 1, gpu), pb.Yref[:, :1]), (kind, v)


# ---------------------------------------------------------------------------
# 7: the reassociating paths at E
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 8, 33])
def test_merge_path(gpu, flat, K):
    """NONZERO, tiles="off": k_merge_flat (K = 32), k_merge + k_carry_fixup
    (K = 8 vectorised, K = 33 scalar), within the tolerance."""
    pb = big()
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD_E, K, dX)
    plan = smfv.SpmmPlan(V.NONZERO, dA, K, tiles="off")
    untiled(plan.stats())
    note(f"merge K={K}", plan.stats())
    assert check_tol(execute(plan, Xv, M, K, gpu), pb, slice(0, K))


def test_mfma(gpu, flat):
    """k_rows_mfma on the finite input at E, within the tolerance."""
    K = 32
    pb = problem(finite=True)
    dA, dX = pb.dev(gpu)
    Xv = x_window(flat, LD_E, K, dX)
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", mfma=True)
    st = plan.stats()
    assert st["mfma"] and st["kernel"] == "k_rows_mfma", st
    assert check_tol(execute(plan, Xv, M, K, gpu), pb, slice(0, K))


# ---------------------------------------------------------------------------
# 8: a row block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("live", [False, True])
def test_row_block(gpu, flat, live):
    """rows = (1001, 2500) at E, K = 32: the tiled snapshot plan (dma16
    instance) and the live plan (the launch_rows fallback from row_begin),
    plain and fused; the block's Y sits in the middle of a NaN buffer."""
    K = 32
    pb = big()
    dA, dX = pb.dev(gpu)
    r0, r1 = ROWS
    Xv = x_window(flat, LD_E, K, dX)
    S, Y0 = pb.Yref[r0:r1, :K], y0()[r0:r1, :K]
    for axpby in (False, True):
        plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", rows=ROWS, live_values=live, axpby=axpby)
        st = plan.stats()
        assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["row_begin"] == r0, st
        assert st["direct_rows"] >= 1 and st["live_values"] == live, st
        assert plan.epilogue_mode == ("fused" if axpby else None)
        Yall = torch.full((M, K), NAN, dtype=torch.float64, device=gpu)
        if axpby:
            Yall[r0:r1] = torch.tensor(Y0)
            plan.run_axpby(Xv, Yall[r0:r1], ALPHA, BETA)
        else:
            plan.run(Xv, Yall[r0:r1])
        torch.cuda.synchronize()
        Yh = Yall.cpu().numpy()
        assert np.isnan(Yh[:r0]).all() and np.isnan(Yh[r1:]).all()
        assert adv.same(Yh[r0:r1], expected(S, Y0) if axpby else S), (live, axpby, st)


# ---------------------------------------------------------------------------
# 9: Y wide (ldy = LD_E: rows >= 2,000 of Y start beyond 2^32)
# ---------------------------------------------------------------------------
def y_wide(flat, plan, Xc, K, Y0=None):
    """Run into the window [G, G + K) of the NaN-filled (M, LD_E) view; every
    element outside the window is still NaN afterwards (checked on the device)."""
    flat.fill_(NAN)
    Yv = flat.view(M, LD_E)[:, G:G + K]
    if Y0 is None:
        plan.run(Xc, Yv)
    else:
        Yv.copy_(torch.tensor(Y0))
        plan.run_axpby(Xc, Yv, ALPHA, BETA)
    torch.cuda.synchronize()
    Yh = Yv.cpu().numpy()
    Yv.fill_(NAN)
    assert bool(torch.isnan(flat).all()), "Y written outside its window"
    return Yh


def _kernel(name, tiled=True, live=False):
    def want(st):
        assert st["tiled"] == tiled and st["kernel"] == name and st["live_values"] == live, st
    return want


Y_WIDE = [  # id, K, problem, variant, plan arguments, stats check, axpby mode, bit-exact
    ("mh-K32", 32, "long", V.ROWWISE, dict(tiles="off"), untiled, None, True),
    ("mh-K128", 128, "long", V.ROWWISE, dict(tiles="off"), untiled, None, True),
    ("rows-K33", 33, "long", V.ROWWISE, dict(tiles="off"), untiled, None, True),
    *[(f"{tk}-K{K}", K, "long", V.ROWWISE, dict(tiles="force", tiled_kernel=tk), ws(tk), None, True)
      for tk in GEOMS for K in (64, 16)],
    ("live-K32", 32, "long", V.ROWWISE, dict(tiles="force", live_values=True), _kernel("k_rows_ws", live=True),
     None, True),
    ("wsn-K8", 8, "long", V.ROWWISE, dict(tiles="force"), _kernel("k_rows_wsn"), None, True),
    ("chunks-K1", 1, "short", V.ROWWISE, dict(), _kernel("k_spmv_chunks"), None, True),
    ("stream-K1", 1, "long", V.ROWWISE, dict(), _kernel(None, tiled=False), None, True),
    ("merge-K32", 32, "long", V.NONZERO, dict(tiles="off"), untiled, None, False),
    ("merge-K8", 8, "long", V.NONZERO, dict(tiles="off"), untiled, None, False),
    ("mfma-K32", 32, "finite", V.ROWWISE, dict(tiles="force", mfma=True), _kernel("k_rows_mfma"), None, False),
    ("fused-ws-K32", 32, "long", V.ROWWISE, dict(tiles="force", axpby=True), _kernel("k_rows_ws"), "fused", True),
    ("fused-mh-K32", 32, "long", V.ROWWISE, dict(tiles="off", axpby=True), untiled, "fused", True),
    ("two-pass-K32", 32, "long", V.ROWWISE, dict(tiles="force", axpby="two_pass"), _kernel("k_rows_ws"),
     "two_pass", True),
]


@pytest.mark.parametrize("K,kind,variant,kw,want,mode,exact", [c[1:] for c in Y_WIDE], ids=[c[0] for c in Y_WIDE])
def test_y_wide(gpu, flat, K, kind, variant, kw, want, mode, exact):
    """One case per kernel family writing Y with ldy = LD_E (Y + (int64_t)row
    * ldy; k_axpby's `row * ldy` with a 64-bit row) from a small contiguous X.
    The fused and two-pass axpby read and write Y in place."""
    pb = {"long": big, "short": lambda: problem("short"), "finite": lambda: problem(finite=True)}[kind]()
    dA, dX = pb.dev(gpu)
    Xc = dX[:, :K].contiguous()
    plan = smfv.SpmmPlan(variant, dA, K, **kw)
    st = plan.stats()
    want(st)
    assert plan.epilogue_mode == mode, (plan.epilogue_mode, st)
    note(f"y-wide K={K} {variant.name} {kw}", st)
    S = pb.Yref[:, :K]
    if mode:
        Y0 = y0()[:, :K]
        assert adv.same(y_wide(flat, plan, Xc, K, Y0), expected(S, Y0)), st
    elif exact:
        Y = y_wide(flat, plan, Xc, K)
        assert adv.same(Y[2000:], S[2000:]), ("rows beyond 2^32", st)
        assert adv.same(Y, S), st
    else:
        assert check_tol(y_wide(flat, plan, Xc, K), pb, slice(0, K)), st
