"""The stream contract of plans (include/smfv.h, "Streams"): bind and execute
are asynchronous on the caller's stream and capture into a hipGraph -- no
allocation, no synchronisation, no launch on another stream, nothing staged on
the host at call time.  Every plan family is captured once on a side stream
(global capture error mode: a hidden allocation, sync or null-stream launch is
an error) and replayed on new X, new Y and, where the plan reads them live,
new values of A; the captured bind + execute sequence bench.py times is
compared with a reference; a capture while the bind's gather is in flight is
refused; multi-launch sequences run in stream order with no device-wide sync;
two merge-path plans run side by side on two streams.

Inputs and references are those of test_gpu_adversarial.py (m = n = 3000,
tests/adversarial.py): adversarial.ref_f64 under adversarial.same for the
bit-exact paths, 1e-12 x sum|a||x| + 1e-300 against the np.longdouble loop for
the reassociating ones (merge path, FMA, MFMA on the finite input).  Every
column of Y depends on the same column of X alone, so a replay on other
columns of the problem's X has its reference in the same columns of Yref.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adversarial as adv
from test_gpu_adversarial import BITWISE, M, Problem, ROWS, V, check_tol, note, problem

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import dist as D
from sparsematrixmultiplicationmpi_amd._lib import SmfvError, call
from sparsematrixmultiplicationmpi_amd.engine import stream_handle

pytestmark = pytest.mark.gpu
G = 2  # NaN guard columns on each side of a Y window (16 bytes: the window stays 16-byte aligned)
ALPHA, BETA = 1.0 / 3.0, -0.7
NAN = float("nan")


# ---------------------------------------------------------------------------
# problems, references, helpers
# ---------------------------------------------------------------------------
def get_problem(kind):
    if kind == "finite":
        return problem(finite=True)
    if kind == "wide":
        return problem("wide", kx=2)  # (n = 80,000: two columns are enough for K = 1)
    return problem(kind)


@functools.lru_cache(maxsize=None)
def reshuffled(kind, which):
    """The problem `kind` with A's values permuted (same pattern, same X): the
    changed values of the live-values replays and of the captured binds.  Its
    references are one more CPU loop each, computed once."""
    pb = get_problem(kind)
    A = pb.A
    perm = np.random.default_rng(100 + which).permutation(A.nnz)
    return Problem(adv.Csr(A.values[perm], A.colIndices, A.rowPtr, A.numRows, A.numCols), pb.X, pb.info)


def private_csr(pb, gpu):
    """A DeviceCSR of the test's own (Problem.dev() is shared and read-only)."""
    A = pb.A
    return smfv.DeviceCSR(smfv.SparseMatrix(A.values, A.colIndices, A.rowPtr, A.numRows, A.numCols), gpu)


def capture(fn):
    """fn(side) captured on a fresh side stream: one stream, no forks, the
    default (global) capture error mode.  Returns (graph, side)."""
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn(side)
    torch.cuda.current_stream().wait_stream(side)
    return g, side


def window(m, K, gpu):
    """A NaN-filled (m, G + K + G) buffer and its window [G, G + K)."""
    Yb = torch.full((m, G + K + G), NAN, dtype=torch.float64, device=gpu)
    return Yb, Yb[:, G:G + K]


def read(Yb, K):
    """The window of Yb on the host; the guard columns must still be NaN."""
    torch.cuda.synchronize()
    Yh = Yb.cpu().numpy()
    assert np.isnan(Yh[:, :G]).all() and np.isnan(Yh[:, G + K:]).all(), "Y written outside its window"
    return np.ascontiguousarray(Yh[:, G:G + K])


def all_nan(T):
    torch.cuda.synchronize()
    return bool(torch.isnan(T).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def second_cols(K, kx):
    """The columns of the second replay: [K, 2K) of the problem's X; where X
    is not that wide (K = 128 of 128), its columns rotated by K / 2."""
    return np.arange(K, 2 * K) if 2 * K <= kx else (np.arange(K) + K // 2) % kx


def agrees(case, Y, pb, cols):
    rows = slice(*case.rows) if case.rows else slice(None)
    if case.tol:
        return check_tol(Y, pb, cols, rows)
    return adv.same(Y, pb.Yref[rows, cols])


@functools.lru_cache(maxsize=None)
def sleep_cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, timed with events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    e1.synchronize()
    return 10_000_000 / max(e0.elapsed_time(e1), 1e-3)


def gpu_sleep(ms):
    """Keep the current stream busy for about `ms` (nothing sleeps on the host)."""
    torch.cuda._sleep(int(ms * sleep_cycles_per_ms()))


# ---------------------------------------------------------------------------
# 1. every plan family, captured once and replayed
# ---------------------------------------------------------------------------
def C(id, kind, K, variant, want, tol=False, xw=None, f=0, rows=None, **kw):
    return pytest.param(SimpleNamespace(id=id, kind=kind, K=K, variant=variant, want=want, tol=tol, xw=xw or K,
                                        f=f, rows=rows, kw=kw), id=id)


some = lambda v: v >= 1  # noqa: E731
UNTILED = {"tiled": False, "kernel": None}


def WS(geom, live):
    return {"tiled": True, "kernel": "k_rows_ws", "ws_geom": geom, "live_values": live, "direct_rows": some}


WSP = lambda geom, live: dict(WS(geom, live), paired_rows=some)  # noqa: E731
WSN = {"tiled": True, "kernel": "k_rows_wsn", "direct_rows": some}
CHUNKS = {"tiled": True, "kernel": "k_spmv_chunks"}

CASES = [
    # untiled rows: k_rows (odd K), k_rows_mh
    C("rows-K3", "long", 3, V.SEQUENTIAL, UNTILED, tiles="off"),
    C("rows_mh-K8", "long", 8, V.ROWWISE, UNTILED, tiles="off"),
    C("rows_mh-K32", "long", 32, V.COLUMNWISE, UNTILED, tiles="off"),
    C("rows_mh-K128", "long", 128, V.ROWWISE, UNTILED, tiles="off"),
    # K = 1: k_spmv_stream, k_spmv_chunks, its 32-bit-column form
    C("k1-stream", "long", 1, V.ROWWISE, UNTILED),
    C("k1-chunks", "short", 1, V.ROWWISE, CHUNKS),
    C("k1-chunks-wide", "wide", 1, V.SEQUENTIAL, CHUNKS),
    # k_rows_ws + k_rows_list: the three geometries, snapshot and live
    C("ws1-snap", "long", 32, V.ROWWISE, WSP(1, False), tiles="force", tiled_kernel="ws1", row_pairs="on"),
    C("ws2-snap", "long", 32, V.SEQUENTIAL, WSP(2, False), tiles="force", tiled_kernel="ws2", row_pairs="on"),
    C("ws3-snap", "long", 32, V.COLUMNWISE, WSP(3, False), tiles="force", tiled_kernel="ws3", row_pairs="on"),
    C("ws1-live", "long", 32, V.COLUMNWISE, WSP(1, True), tiles="force", tiled_kernel="ws1", row_pairs="on",
      live_values=True),
    C("ws2-live", "long", 32, V.ROWWISE, WSP(2, True), tiles="force", tiled_kernel="ws2", row_pairs="on",
      live_values=True),
    C("ws3-live", "long", 32, V.SEQUENTIAL, WSP(3, True), tiles="force", tiled_kernel="ws3", row_pairs="on",
      live_values=True),
    C("ws2-snap-K64", "long", 64, V.ROWWISE, WSP(2, False), tiles="force", tiled_kernel="ws2", row_pairs="on"),
    # NARROW: the window [16, 32) of a 32-wide X
    C("narrow-snap", "long", 16, V.ROWWISE, WS(1, False), xw=32, f=16, tiles="force", tiled_kernel="ws1"),
    C("narrow-live", "long", 16, V.ROWWISE, WS(3, True), xw=32, f=16, tiles="force", tiled_kernel="ws3",
      live_values=True),
    # k_rows_wsn: a window of 4 / 8 columns of a 32-wide X
    C("wsn-K4", "long", 4, V.ROWWISE, WSN, xw=32, f=24, tiles="force"),
    C("wsn-K8", "long", 8, V.COLUMNWISE, WSN, xw=32, f=20, tiles="force"),
    # the opt-ins, on the finite input
    C("fma-K32", "finite", 32, V.ROWWISE, {"tiled": True, "kernel": "k_rows_ws"}, tol=True, tiles="force", fma=True),
    C("mfma-K32", "finite", 32, V.ROWWISE, {"mfma": True, "kernel": "k_rows_mfma"}, tol=True, tiles="force",
      mfma=True),
    # NONZERO: k_merge_flat, k_merge vectorised / scalar (+ k_carry_fixup); the tiled kernel over whole rows
    C("merge_flat-K32", "long", 32, V.NONZERO, UNTILED, tol=True, tiles="off"),
    C("merge-K8", "long", 8, V.NONZERO, UNTILED, tol=True, tiles="off"),
    C("merge-K33", "long", 33, V.NONZERO, UNTILED, tol=True, tiles="off"),
    C("nonzero-tiled-K32", "long", 32, V.NONZERO, {"tiled": True, "kernel": "k_rows_ws", "direct_rows": some},
      tiles="force"),
    # plans of the row block [1001, 2500)
    C("rowblock-K32", "long", 32, V.ROWWISE,
      {"tiled": True, "kernel": "k_rows_ws", "row_begin": ROWS[0], "direct_rows": some}, rows=ROWS, tiles="force"),
    C("rowblock-K1", "long", 1, V.ROWWISE, dict(UNTILED, row_begin=ROWS[0]), rows=ROWS, tiles="force"),
]


@pytest.mark.parametrize("case", CASES)
def test_capture_replay(gpu, case):
    """One run() captured, then replayed on the first K columns of X, on other
    columns written into the same X buffer (Y refilled with NaN), once more
    without refilling (same bits) and -- a plan that reads A's values live --
    on values changed in place.  Capture itself executes nothing; nothing is
    written outside the Y window; X outside the plan's window is NaN."""
    K, f = case.K, case.f
    pb = get_problem(case.kind)
    assert case.variant in BITWISE or case.variant == V.NONZERO
    _, dXall = pb.dev(gpu)
    kx = pb.X.shape[1]
    cols1, cols2 = np.arange(K), second_cols(K, kx)
    # the plan: built once, on the stream it will not run on
    dA = private_csr(pb, gpu)
    plan = smfv.SpmmPlan(case.variant, dA, K, rows=case.rows, **case.kw)
    st = plan.stats()
    for key, want in case.want.items():
        assert want(st[key]) if callable(want) else st[key] == want, (key, st)
    note(f"capture {case.id} {case.variant.name}", st)
    live = not st["tiled"] or st["live_values"]
    # X: the window [f, f + K) of an xw-wide buffer, NaN outside the window
    Xb = torch.full((pb.A.numCols, case.xw), NAN, dtype=torch.float64, device=gpu)
    Xw = Xb[:, f:f + K]
    Xw.copy_(dXall[:, torch.from_numpy(cols1).to(gpu)])
    Yb, Yw = window(plan.m_out, K, gpu)
    g, side = capture(lambda s: plan.run(Xw, Yw, stream=s))
    assert all_nan(Yb), "the capture executed"
    g.replay()
    assert agrees(case, read(Yb, K), pb, cols1), (case.id, st)
    # other columns, written in place into the captured X
    Xw.copy_(dXall[:, torch.from_numpy(cols2).to(gpu)])
    Yb.fill_(NAN)
    g.replay()
    assert agrees(case, read(Yb, K), pb, cols2), (case.id, "second X", st)
    before = Yb.clone()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(Yb, before), (case.id, "replay without refilling")
    if live:
        pb2 = reshuffled(case.kind, 1)
        dA.values.copy_(torch.from_numpy(pb2.A.values))
        Yb.fill_(NAN)
        g.replay()
        assert agrees(case, read(Yb, K), pb2, cols2), (case.id, "values changed in place", st)
    del g


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("variant", [V.COLUMNWISE, V.NONZERO], ids=lambda v: v.name)
def test_capture_rank_plan(gpu, variant, r):
    """run_local of every rank's plan at p = 3 (COLUMNWISE: the rank's column
    panel; NONZERO: its whole rows by the tiled sub-plan, its cut rows by
    k_cut_rows), captured and replayed: the bits of one eager run_local in the
    exchange buffer and in Y (test_gpu_adversarial.test_rank_plans checks the
    eager result)."""
    K, p = 32, 3
    pb = problem()
    dA, dX = pb.dev(gpu)
    dX32 = dX[:, :K].contiguous()
    P = D.DistPlan(None, variant, dA, K, to_all=False, root=2, tiles="force", rank=(r, p))
    print("PATH capture rank plan", variant.name, r, P.stats())
    buf = P.exchange_buffer()
    assert buf is not None
    Y = torch.full((M, K), NAN, dtype=torch.float64, device=gpu)
    buf.fill_(NAN)
    P.run_local(dX32, Y)
    torch.cuda.synchronize()
    eager_buf, eager_Y = buf.clone(), Y.clone()
    assert not all_nan(eager_buf), "run_local wrote nothing"
    buf.fill_(NAN)
    Y.fill_(NAN)
    g, side = capture(lambda s: P.run_local(dX32, Y, stream=s))
    assert all_nan(buf) and all_nan(Y), "the capture executed"
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(buf, eager_buf) and same_bits(Y, eager_Y), (variant, r)
        buf.fill_(NAN)
        Y.fill_(NAN)
    del g


def axpby_problem():
    """The finite problem, a Y0 and the tolerance of a reassociated
    alpha * A X + beta * Y0 at K = 8 (test_gpu_axpby.py's: 1e-12 x (|alpha|
    sum|a||x| + |beta||y0|) + 1e-300); every element's scale is finite."""
    pb = problem(finite=True)
    K = 8
    Y0 = np.random.default_rng(7).uniform(-1, 1, (M, K))
    assert np.isfinite(pb.scale).all() and pb.scale.max() < 1e300

    def ok(Y, cols):
        want = np.longdouble(ALPHA) * pb.Yhi[:, cols] + np.longdouble(BETA) * Y0
        bound = 1e-12 * (abs(ALPHA) * pb.scale[:, cols] + abs(BETA) * np.abs(Y0)) + np.longdouble(1e-300)
        err = np.abs(Y.astype(np.longdouble) - want)
        print("TOL worst error / bound", float(np.max(err / bound)))
        return bool(np.all(err <= bound))
    return pb, K, Y0, ok


def test_capture_two_pass_axpby(gpu):
    """run_axpby of a NONZERO merge-path plan (k_merge + k_carry_fixup into the
    plan's scratch, then k_axpby), captured and replayed on two X."""
    pb, K, Y0, ok = axpby_problem()
    dA, dXall = pb.dev(gpu)
    plan = smfv.SpmmPlan(V.NONZERO, dA, K, tiles="off", axpby=True)
    assert plan.epilogue_mode == "two_pass" and not plan.stats()["tiled"], plan.stats()
    note("capture two-pass axpby merge K=8", plan.stats())
    dX = dXall[:, :K].contiguous()
    dY0 = torch.from_numpy(Y0).to(gpu)
    Yb, Yw = window(M, K, gpu)
    g, side = capture(lambda s: plan.run_axpby(dX, Yw, ALPHA, BETA, stream=s))
    assert all_nan(Yb), "the capture executed"
    for cols in (np.arange(K), np.arange(K, 2 * K)):
        dX.copy_(dXall[:, int(cols[0]):int(cols[-1]) + 1])
        Yw.copy_(dY0)
        g.replay()
        assert ok(read(Yb, K), cols), cols[0]
    del g


# ---------------------------------------------------------------------------
# 2. captured bind + execute: the sequence bench.py's rebind leg times
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,f,descriptors,kw", [
    ("ws", 32, 0, True, {"row_pairs": "on"}),  # binds by k_bind_items
    ("wsn", 8, 20, False, {}),                 # binds by k_gather_vals
], ids=["ws-bind_items", "wsn-gather_vals"])
def test_captured_bind_execute(gpu, kind, K, f, descriptors, kw):
    """bind(va), execute(va -> Ya), bind(vb), execute(vb -> Yb) captured through
    the C calls: the gathers run at replay (va changed in place between two
    replays is followed), and afterwards the plan serves eager calls -- an
    execute with vb, the last values bound, on the non-capture stream, then a
    bind + run with the current values."""
    pb, pbb, pbc = problem(), reshuffled("long", 1), reshuffled("long", 2)
    cols = slice(f, f + K)
    _, dXall = pb.dev(gpu)
    dX32 = dXall[:, :32].contiguous()
    Xw = dX32[:, cols]
    dA = private_csr(pb, gpu)
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force", **kw)
    st = plan.stats()
    assert st["tiled"] and not st["live_values"] and st["direct_rows"] >= 1, st
    assert st["kernel"] == {"ws": "k_rows_ws", "wsn": "k_rows_wsn"}[kind] and st["bind_descriptors"] == descriptors, st
    note(f"captured bind {kind} bind_descriptors={st['bind_descriptors']}", st)
    va = dA.values
    vb, vc = (torch.from_numpy(q.A.values).to(gpu) for q in (pbb, pbc))
    (Yab, Ya), (Ybb, Yb) = window(M, K, gpu), window(M, K, gpu)
    rp, ci, _ = dA.ptrs()

    def execute(vals, Y, s):
        call("smfv_plan_execute", plan._plan, rp, ci, vals.data_ptr(), Xw.data_ptr(), 32, Y.data_ptr(), Y.stride(0),
             stream_handle(s))

    def steps(s):
        for vals, Y in ((va, Ya), (vb, Yb)):
            call("smfv_plan_bind_values", plan._plan, vals.data_ptr(), stream_handle(s))
            execute(vals, Y, s)
    g, side = capture(steps)
    assert all_nan(Yab) and all_nan(Ybb), "the capture executed"
    g.replay()
    assert adv.same(read(Yab, K), pb.Yref[:, cols]) and adv.same(read(Ybb, K), pbb.Yref[:, cols]), st
    # the gather runs at replay: va's new contents are followed, vb's result is rewritten
    va.copy_(vc)
    Yab.fill_(NAN)
    Ybb.fill_(NAN)
    g.replay()
    assert adv.same(read(Yab, K), pbc.Yref[:, cols]) and adv.same(read(Ybb, K), pbb.Yref[:, cols]), st
    # eager, on the current stream, with the values the captured sequence bound last
    torch.cuda.synchronize()
    Ybb.fill_(NAN)
    execute(vb, Yb, None)
    assert adv.same(read(Ybb, K), pbb.Yref[:, cols]), "eager execute after a captured bind"
    # eager bind + run with the current values (bench.py after its rebind leg)
    plan.bind_values()
    Yab.fill_(NAN)
    plan.run(Xw, Ya)
    assert adv.same(read(Yab, K), pbc.Yref[:, cols]), "eager bind + run after a captured bind"
    del g


# ---------------------------------------------------------------------------
# 3. capture while the bind's gather is in flight
# ---------------------------------------------------------------------------
def test_capture_while_bind_in_flight(gpu):
    """A snapshot plan bound on a stream that is still busy: capturing an
    execute on another stream is refused before any launch (SmfvError, the
    snapshot is still in flight), the capture unwinds, and after the bind
    stream has drained a fresh capture of the same plan replays the
    reference.  (torch.cuda.graph synchronises the device on entry, so the
    busy bind is issued inside the capture region, on its own stream.)"""
    K = 32
    pb = problem()
    dA, dXall = pb.dev(gpu)
    dX = dXall[:, :K].contiguous()
    plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force")
    st = plan.stats()
    assert st["tiled"] and not st["live_values"], st
    Yb, Yw = window(M, K, gpu)
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
    assert adv.same(read(Yb, K), pb.Yref[:, :K]), st
    del g


# ---------------------------------------------------------------------------
# 4. stream order without a device-wide sync
# ---------------------------------------------------------------------------
def in_stream_order(s, dX, Xsrc, launch, Ysrc, gpu):
    """On the side stream s alone: a sleep, X (NaN so far) written, the
    launches, the result copied out; the host waits once, for s.  A launch
    that left s (torch's side streams do not synchronise with the null
    stream) would read the NaN X or write after the copy."""
    Yout = torch.full_like(Ysrc, NAN)
    sleep_cycles_per_ms()  # (timed here, not inside the sequence)
    torch.cuda.synchronize()  # (the set-up, on the current stream, is done)
    with torch.cuda.stream(s):
        gpu_sleep(20)
        dX.copy_(Xsrc)
        launch(s)
        Yout.copy_(Ysrc)
    s.synchronize()
    return Yout


@pytest.mark.parametrize("what", ["merge-K8", "ws-direct-rows", "bound-elsewhere", "two-pass-axpby"])
def test_stream_order(gpu, what):
    """The multi-launch sequences, eagerly on one side stream, checked after
    s.synchronize() alone: k_merge + k_carry_fixup; k_rows_ws + k_rows_list;
    a snapshot re-bound on another, busy stream just before (the execute's
    hipStreamWaitEvent: without it the stale snapshot would be used); merge
    path + k_axpby."""
    s = torch.cuda.Stream()
    keep = []
    if what == "two-pass-axpby":
        pb, K, Y0, ok = axpby_problem()
    else:
        pb, K = problem(), 8 if what == "merge-K8" else 32
    want = pb
    _, dXall = pb.dev(gpu)
    Xsrc = dXall[:, :K].contiguous()
    dX = torch.full_like(Xsrc, NAN)
    Yb, Yw = window(M, K, gpu)
    if what == "merge-K8":
        plan = smfv.SpmmPlan(V.NONZERO, pb.dev(gpu)[0], K, tiles="off")
        assert not plan.stats()["tiled"]
        launch = lambda st: plan.run(dX, Yw, stream=st)  # noqa: E731
    elif what == "ws-direct-rows":
        plan = smfv.SpmmPlan(V.ROWWISE, pb.dev(gpu)[0], K, tiles="force", stream=s)
        assert plan.stats()["kernel"] == "k_rows_ws" and plan.stats()["direct_rows"] >= 1, plan.stats()
        launch = lambda st: plan.run(dX, Yw, stream=st)  # noqa: E731
    elif what == "bound-elsewhere":
        dA = private_csr(pb, gpu)
        plan = smfv.SpmmPlan(V.ROWWISE, dA, K, tiles="force")
        assert plan.stats()["kernel"] == "k_rows_ws" and not plan.stats()["live_values"], plan.stats()
        want = reshuffled("long", 1)
        dA.values.copy_(torch.from_numpy(want.A.values))
        s_bind = torch.cuda.Stream()
        keep.append(s_bind)

        def launch(st):
            with torch.cuda.stream(s_bind):  # the new snapshot, behind a sleep on another stream
                gpu_sleep(20)
            plan.bind_values(s_bind)
            plan.run(dX, Yw, stream=st)
    else:
        plan = smfv.SpmmPlan(V.NONZERO, pb.dev(gpu)[0], K, tiles="off", axpby=True)
        assert plan.epilogue_mode == "two_pass"
        Yw.copy_(torch.from_numpy(Y0).to(gpu))
        launch = lambda st: plan.run_axpby(dX, Yw, ALPHA, BETA, stream=st)  # noqa: E731
    note(f"stream order {what}", plan.stats())
    Yout = in_stream_order(s, dX, Xsrc, launch, Yb, gpu)
    for t in keep:
        t.synchronize()
    Y = read(Yout, K)
    if what == "two-pass-axpby":
        assert ok(Y, np.arange(K))
    elif what == "merge-K8":
        assert check_tol(Y, want, slice(0, K))
    else:
        assert adv.same(Y, want.Yref[:, :K]), what


def test_stream_order_rank_plan_cut_rows(gpu):
    """The NONZERO plan of rank 1 of 3 (its first and last rows are shared
    with its neighbours: tiled sub-plan + k_cut_rows) in stream order: the
    bits of its eager run_local."""
    K, p, r = 32, 3, 1
    pb = problem()
    A = pb.A
    first, last, _, _ = D.exchange_plan(V.NONZERO, M, A.nnz, A.rowPtr, K, p, D.dist_opts("reference"))
    assert last[r - 1] == first[r] and last[r] == first[r + 1], (first, last)  # both ends cut
    dA, dXall = pb.dev(gpu)
    Xsrc = dXall[:, :K].contiguous()
    P = D.DistPlan(None, V.NONZERO, dA, K, to_all=False, root=2, tiles="force", rank=(r, p))
    print("PATH stream order rank plan", P.stats())
    buf = P.exchange_buffer()
    Y = torch.full((M, K), NAN, dtype=torch.float64, device=gpu)
    buf.fill_(NAN)
    P.run_local(Xsrc, Y)
    torch.cuda.synchronize()
    eager = buf.clone()
    assert not all_nan(eager)
    buf.fill_(NAN)
    dX = torch.full_like(Xsrc, NAN)
    s = torch.cuda.Stream()
    out = in_stream_order(s, dX, Xsrc, lambda st: P.run_local(dX, Y, stream=st), buf, gpu)
    assert same_bits(out, eager)


# ---------------------------------------------------------------------------
# 5. two plans, two streams
# ---------------------------------------------------------------------------
def test_two_merge_plans_two_streams(gpu):
    """Two merge-path plans (K = 8 and K = 32) of one matrix launched back to
    back on two streams, five rounds with no sync in between (both streams
    start behind a sleep, so their queues drain together): each round's Y has
    the bits of that plan's own single-stream result -- a plan's carry
    workspace is its own."""
    pb = problem()
    dA, dXall = pb.dev(gpu)
    rounds = 5
    plans, X, alone, Ys = {}, {}, {}, {}
    for K in (8, 32):
        plans[K] = smfv.SpmmPlan(V.NONZERO, dA, K, tiles="off")
        assert not plans[K].stats()["tiled"]
        note(f"two streams merge K={K}", plans[K].stats())
        X[K] = dXall[:, :K].contiguous()
        Yb, Yw = window(M, K, gpu)
        plans[K].run(X[K], Yw)
        assert check_tol(read(Yb, K), pb, slice(0, K))
        alone[K] = Yb
        Ys[K] = [window(M, K, gpu) for _ in range(rounds)]
    streams = {8: torch.cuda.Stream(), 32: torch.cuda.Stream()}
    sleep_cycles_per_ms()
    torch.cuda.synchronize()
    for K, s in streams.items():
        with torch.cuda.stream(s):
            gpu_sleep(5)
    for i in range(rounds):
        for K, s in streams.items():
            plans[K].run(X[K], Ys[K][i][1], stream=s)
    for s in streams.values():
        s.synchronize()
    for K in (8, 32):
        for i in range(rounds):
            assert same_bits(Ys[K][i][0], alone[K]), (K, i)
