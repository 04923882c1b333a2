"""The block-vector family on the GPU (smfv_coldot_f64, smfv_col_axpy_f64,
smfv_col_xpay_f64, smfv_pcg_update_f64, BlockPCG): every comparison is bit for
bit through an int64 view against the numpy restatement of the rules in
tests/blockvec_ref.py (never the library); where a NaN is the expected result
only its position is compared (payloads are not promised).
"""
import numpy as np
import pytest
import torch

import blockvec_ref as BR
from test_gpu_capture import NAN, capture, in_stream_order
from test_gpu_reorder import BIG_F, BIG_LD, BIG_M, big_buffer, csr_of  # noqa: F401  (big_buffer is a fixture)

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd._lib import SmfvError

pytestmark = pytest.mark.gpu
GUARD = 16  # NaN doubles on each side of a small buffer
MS = [0, 1, 31, 33, 511, 512, 513, 1025, 2600]  # a strand edge, a chunk edge, a short last chunk, six chunks
KS = [1, 2, 3, 8, 31, 32, 40, 64, 128]  # every team width, both access widths


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """Equal bit for bit; where b is NaN, a must be NaN (any payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


def uniform(m, K, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (m, K))


class Window:
    """An m x K block as a window of a NaN-filled flat buffer: leading
    dimension ld >= K, `shift` doubles off a 16-byte boundary, a guard band on
    both sides.  read() returns the block and insists that the padding and the
    guards are still NaN."""

    def __init__(self, Xh, ld, shift, gpu):
        Xh = np.asarray(Xh, np.float64)
        self.m, self.K = Xh.shape
        self.ld = ld
        g = 2 * GUARD + shift
        self.buf = torch.full((g + self.m * ld + 2 * GUARD,), NAN, dtype=torch.float64, device=gpu)
        self.v = self.buf[g:g + self.m * ld].view(self.m, ld)[:, :self.K]
        assert self.m == 0 or (self.v.data_ptr() % 16 == 0) == (shift % 2 == 0)  # (an empty view has no address)
        self.v.copy_(torch.from_numpy(Xh))
        self.idx = g + (np.arange(self.m)[:, None] * ld + np.arange(self.K)[None, :]).reshape(-1)

    def read(self):
        h = self.buf.cpu().numpy()
        win = np.zeros(h.size, bool)
        win[self.idx] = True
        assert np.isnan(h[~win]).all(), "written outside the K columns"
        return h[self.idx].reshape(self.m, self.K)


def cols(vh, gpu, shift=0):
    """K per-column doubles inside a NaN band: (buffer, view)."""
    vh = np.asarray(vh, np.float64)
    buf = torch.full((2 * GUARD + shift + vh.size + GUARD,), NAN, dtype=torch.float64, device=gpu)
    v = buf[2 * GUARD + shift:2 * GUARD + shift + vh.size]
    v.copy_(torch.from_numpy(vh))
    return buf, v


def band_ok(buf, v):
    """Everything of buf outside the view v is still NaN."""
    h = buf.cpu().numpy()
    lo = (v.data_ptr() - buf.data_ptr()) // 8
    return bool(np.isnan(h[:lo]).all() and np.isnan(h[lo + v.numel():]).all())


def run_coldot(Xh, Yh, gpu, ldx, ldy, shift=0, x_is_y=False):
    """coldot with X, Y, out and a NaN-prefilled workspace as windows of
    NaN-filled buffers; the guards, the padding and the inputs are checked."""
    m, K = Xh.shape
    X = Window(Xh, ldx, shift, gpu)
    Y = X if x_is_y else Window(Yh, ldy, shift, gpu)
    obuf, out = cols(np.full(K, NAN), gpu, shift)
    wbuf, ws = cols(np.full(smfv.engine.coldot_workspace_doubles(m, K), NAN), gpu)
    got = smfv.coldot(X.v, Y.v, out=out, workspace=ws)
    assert got is out
    torch.cuda.synchronize()
    assert band_ok(obuf, out) and band_ok(wbuf, ws), "written outside out / the workspace"
    assert same_bits(X.read(), Xh) and same_bits(Y.read(), Xh if x_is_y else Yh), "an input changed"
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# coldot
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("m", MS)
def test_coldot(gpu, m, K):
    """Against the vectorised rule: contiguous (16-byte accesses at even K),
    ld > K (odd and even padding), views one double off alignment (the 8-byte
    path at even K too), X is Y; the workspace starts as NaN; no result is
    -0.0.  On these inputs a row-sequential sum gives other bits."""
    X, Y = uniform(m, K, 1000 * m + K), uniform(m, K, 1000 * m + K + 500)
    want = BR.coldot(X, Y)
    if m >= 31 and K >= 3:
        assert not np.array_equal(bits(want), bits(BR.rowseq_dot(X, Y)))
    for ldx, ldy, shift in ((K, K, 0), (K + 6, K + 2, 0), (K + 3, K + 5, 0), (K + 2, K + 2, 1), (K + 1, K + 4, 1)):
        got = run_coldot(X, Y, gpu, ldx, ldy, shift)
        assert same_bits(got, want), (ldx, ldy, shift)
        assert not (np.signbit(got) & (got == 0)).any()  # never -0.0
    got = run_coldot(X, None, gpu, K + 2, K + 2, 0, x_is_y=True)
    assert same_bits(got, BR.coldot(X, X))
    if m == 0:
        assert np.array_equal(bits(got), np.zeros(K, np.int64))  # +0.0


def special_blocks():
    """m = 1100 (three chunks), one column per case; returns X, Y and the
    expected class of every column."""
    m, K = 1100, 12
    X, Y = uniform(m, K, 7), uniform(m, K, 8)
    inf = np.inf
    X[5, 0] = NAN                                  # NaN in
    X[40, 1], Y[40, 1] = inf, 2.0                  # +inf
    X[700, 2], Y[700, 2] = -inf, 3.0               # -inf
    X[9, 3], Y[9, 3] = inf, 0.0                    # inf * 0
    X[0, 4], Y[0, 4], X[1, 4], Y[1, 4] = inf, 1.0, -inf, 1.0      # inf - inf across strands of a chunk
    X[0, 5], Y[0, 5], X[600, 5], Y[600, 5] = inf, 1.0, -inf, 1.0  # ... across chunks
    X[:, 6], Y[:, 6] = X[:, 6] * 1e-160, Y[:, 6] * 1e-160         # subnormal products
    X[77, 7], Y[77, 7] = 2.0 ** 600, 2.0 ** 600    # overflow
    X[:, 8], Y[:, 8] = X[:, 8] * 2.0 ** 600, Y[:, 8] * 2.0 ** -600
    X[:, 9], Y[:, 9] = 0.0, 1.0
    X[0, 9], X[32, 9], Y[32, 9] = 0.75, 0.75, -1.0  # strand 0: +0.75, then -0.75: exactly +0.0
    X[:, 10], Y[:, 10] = -1.0, 0.0                  # every product is -0.0
    X[:, 11], Y[:, 11] = X[:, 11] * 2.0 ** -600, Y[:, 11] * 2.0 ** -600  # products underflow to zero
    return X, Y


def test_coldot_special_values(gpu):
    X, Y = special_blocks()
    want = BR.coldot(X, Y)
    assert np.isnan(want[[0, 3, 4, 5]]).all() and want[1] == np.inf and want[2] == -np.inf and want[7] == np.inf
    assert 0 < want[6] < 2.3e-308 and np.isfinite(want[8]) and want[8] != 0
    assert np.array_equal(bits(want[[9, 10]]), [0, 0]) and want[11] == 0 and not np.signbit(want[11])
    for ld, shift in ((12, 0), (13, 1)):
        got = run_coldot(X, Y, gpu, ld, ld, shift)
        assert same_bits(got, want), (got, want)
        assert not (np.signbit(got) & (got == 0)).any()  # never -0.0


def test_large_offsets(gpu, big_buffer):
    """m = 70 with a leading dimension of 8.95 million doubles: the last ten
    rows lie beyond 4 GiB.  coldot with X, then Y, as the column window of the
    large buffer; the fused update with P (read), then R (written, two guard
    columns on each side still NaN) there."""
    K = 32
    assert 59 * BIG_LD * 8 < 1 << 32 <= 60 * BIG_LD * 8
    big = big_buffer.view(BIG_M, BIG_LD)
    wide = big[:, BIG_F - 2:BIG_F + K + 2]
    win = big[:, BIG_F:BIG_F + K]
    A, B = uniform(BIG_M, K, 70), uniform(BIG_M, K, 71)
    dB = torch.from_numpy(B).to(gpu)
    win.copy_(torch.from_numpy(A))
    want = BR.coldot(A, B)
    assert same_bits(smfv.coldot(win, dB).cpu().numpy(), want)
    assert same_bits(smfv.coldot(dB, win).cpu().numpy(), want)
    # the fused update
    P, Q, X, R = (uniform(BIG_M, K, 72 + i) for i in range(4))
    num, den = np.random.default_rng(5).uniform(0.5, 2, K), np.random.default_rng(6).uniform(0.5, 2, K)
    Xn, Rn, rr = BR.pcg_update(num, den, 0, P, Q, X, R)
    dnum, dden = torch.from_numpy(num).to(gpu), torch.from_numpy(den).to(gpu)
    dev = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    win.copy_(torch.from_numpy(P))
    dX, dR = dev(X), dev(R)
    got = smfv.pcg_update(dnum, dden, win, dev(Q), dX, dR)
    assert same_bits(got.cpu().numpy(), rr) and same_bits(dX.cpu().numpy(), Xn) and same_bits(dR.cpu().numpy(), Rn)
    wide.fill_(NAN)
    win.copy_(torch.from_numpy(R))
    dX = dev(X)
    got = smfv.pcg_update(dnum, dden, dev(P), dev(Q), dX, win)
    h = wide.cpu().numpy()
    assert np.isnan(h[:, :2]).all() and np.isnan(h[:, -2:]).all(), "written outside R's window"
    assert same_bits(got.cpu().numpy(), rr) and same_bits(dX.cpu().numpy(), Xn) and same_bits(h[:, 2:-2], Rn)


# ---------------------------------------------------------------------------
# axpy, xpay
# ---------------------------------------------------------------------------
def scalars(K, seed, zeros):
    rng = np.random.default_rng(seed)
    num, den = rng.uniform(-2, 2, K), rng.uniform(0.5, 2, K) * rng.choice([-1.0, 1.0], K)
    if zeros:  # 0 / 0, x / 0, x / -0.0
        den[::3] = 0.0
        num[0] = 0.0
        if K > 3:
            den[3] = -0.0
    return num, den


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("m", [1, 33, 257, 1025])
def test_axpy_xpay(gpu, m, K):
    """Both updates against numpy: every flag combination, den NULL, den with
    zeros (+0.0 and -0.0) with and without the guard, padded and misaligned
    windows (padding and guards still NaN, X unchanged), in place."""
    X, Y = uniform(m, K, 31 * m + K), uniform(m, K, 31 * m + K + 7)
    for fn, ref in ((smfv.col_axpy, BR.axpy), (smfv.col_xpay, BR.xpay)):
        for flags in range(4):
            for kind in ("none", "plain", "zeros"):
                num, den = scalars(K, K + flags, kind == "zeros")
                den = None if kind == "none" else den
                ldx, ldy, shift = ((K, K, 0), (K + 3, K + 5, 0), (K + 2, K + 2, 1), (K + 6, K + 2, 0))[flags]
                wx, wy = Window(X, ldx, shift, gpu), Window(Y, ldy, shift, gpu)
                nb, dn = cols(num, gpu, shift)
                db, dd = cols(den, gpu, shift) if den is not None else (None, None)
                out = fn(dn, dd, wx.v, wy.v, negate=bool(flags & 1), zero_den=bool(flags & 2))
                assert out is wy.v
                torch.cuda.synchronize()
                want = ref(num, den, flags, X, Y)
                assert same_bits(wy.read(), want), (fn.__name__, flags, kind)
                assert same_bits(wx.read(), X) and same_bits(dn.cpu().numpy(), num) and band_ok(nb, dn)
                if kind == "zeros" and flags & 2:
                    assert np.isfinite(wy.read()).all()
                if kind == "zeros" and not flags & 2:
                    assert not np.isfinite(wy.read()[:, 0]).any()  # 0 / 0
        # in place: Y is X
        num, den = scalars(K, 99, False)
        w = Window(X, K + 2, 0, gpu)
        fn(cols(num, gpu)[1], cols(den, gpu)[1], w.v, w.v)
        torch.cuda.synchronize()
        assert same_bits(w.read(), ref(num, den, 0, X, X)), fn.__name__


# ---------------------------------------------------------------------------
# the fused update
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 32, 40])
@pytest.mark.parametrize("m", [0, 1, 513, 2600])
def test_pcg_update(gpu, m, K):
    """The fused pass equals the three separate device calls and the numpy
    rules bit for bit: contiguous, padded and misaligned windows, every flag
    combination, den with zeros under the guard."""
    P, Q, X, R = (uniform(m, K, 11 * m + K + i) for i in range(4))
    for flags, (ld, shift) in enumerate(((K, 0), (K + 3, 0), (K + 2, 1), (K + 6, 0))):
        num, den = scalars(K, m + flags, zeros=bool(flags & 2))
        neg, zd = bool(flags & 1), bool(flags & 2)
        wp, wq, wx, wr = (Window(a, ld + 2 * i, shift, gpu) for i, a in enumerate((P, Q, X, R)))
        dn, dd = cols(num, gpu)[1], cols(den, gpu)[1]
        rbuf, rr = cols(np.full(K, NAN), gpu)
        wbuf, ws = cols(np.full(smfv.engine.coldot_workspace_doubles(m, K), NAN), gpu)
        got = smfv.pcg_update(dn, dd, wp.v, wq.v, wx.v, wr.v, rr=rr, negate=neg, zero_den=zd, workspace=ws)
        assert got is rr
        # the three separate calls on copies
        sx, sr = Window(X, ld, shift, gpu), Window(R, ld, shift, gpu)
        smfv.col_axpy(dn, dd, wp.v, sx.v, negate=neg, zero_den=zd)
        smfv.col_axpy(dn, dd, wq.v, sr.v, negate=not neg, zero_den=zd)
        sep = smfv.coldot(sr.v, sr.v)
        torch.cuda.synchronize()
        assert band_ok(rbuf, rr) and band_ok(wbuf, ws)
        Xn, Rn, want = BR.pcg_update(num, den, flags, P, Q, X, R)
        assert same_bits(wx.read(), Xn) and same_bits(wr.read(), Rn) and same_bits(rr.cpu().numpy(), want), flags
        assert same_bits(sx.read(), Xn) and same_bits(sr.read(), Rn) and same_bits(sep.cpu().numpy(), want), flags
        assert same_bits(wp.read(), P) and same_bits(wq.read(), Q)


# ---------------------------------------------------------------------------
# BlockPCG
# ---------------------------------------------------------------------------
def make_pcg(gpu, K, kind):
    dA = csr_of(BR.laplacian(), gpu)
    M = None if kind is None else smfv.Ilu0Preconditioner(dA, K, reorder=None if kind == "natural" else "multicolor")
    return smfv.BlockPCG(dA, K, M)


def state(pcg):
    torch.cuda.synchronize()
    return {k: getattr(pcg, k).cpu().numpy() for k in ("X", "R", "P", "rr")}


def same_state(got, want):
    return all(same_bits(got[k], want[k]) for k in ("X", "R", "P", "rr"))


@pytest.mark.parametrize("kind", [None, "natural", "multicolor"])
@pytest.mark.parametrize("K", [3, 32])
def test_pcg_five_iterations(gpu, K, kind):
    """X, R, P and rr after five iterations equal the numpy loop bit for bit;
    with X0 given too."""
    pcg = make_pcg(gpu, K, kind)
    B = torch.from_numpy(np.array(BR.rhs(K))).to(gpu)
    pcg.start(B)
    pcg.iterate(5)
    want = BR.pcg_iterations(K, kind, 5)
    assert same_state(state(pcg), want)
    assert same_bits(pcg.bb.cpu().numpy(), want["bb"])
    assert np.isfinite(want["X"]).all() and want["rr"].max() < want["bb"].min()  # it is converging
    pcg.start(B, torch.from_numpy(np.array(BR.x0(K))).to(gpu))
    pcg.iterate(2)
    pcg.iterate(3)
    assert same_state(state(pcg), BR.pcg_iterations(K, kind, 5, True))
    assert pcg.iterations == 5


@pytest.mark.parametrize("kind", [None, "multicolor"])
def test_pcg_solve(gpu, kind):
    """solve: the iteration count and rr / bb equal the numpy loop's; a zero
    right-hand-side column stays exactly zero (and finite) while the others
    converge; X0 given; a captured solve equals the launched one."""
    K, tol = 32, 1e-8
    pcg = make_pcg(gpu, K, kind)
    B = torch.from_numpy(np.array(BR.rhs(K, 4))).to(gpu)
    X, its, rel = pcg.solve(B, tol=tol, max_iters=200)
    Xw, itw, relw = BR.pcg_solve(K, kind, tol, 200, False, 4)
    Xh = X.cpu().numpy()
    assert its == itw and 3 < its < 200 and same_bits(rel, relw) and same_bits(Xh, Xw)
    assert np.array_equal(bits(Xh[:, 4]), np.zeros(900, np.int64)) and rel[4] == 0.0 and np.isfinite(Xh).all()
    assert (np.delete(rel, 4) <= tol * tol).all() and (np.delete(rel, 4) > 0).all()
    Xg, itg, relg = pcg.solve(B, tol=tol, max_iters=200, graph=True)
    assert itg == its and same_bits(relg, rel) and same_bits(Xg.cpu().numpy(), Xh)
    # X0 given (a right-hand side without the zero column: X0's column there would never meet rr <= 0)
    B = torch.from_numpy(np.array(BR.rhs(K))).to(gpu)
    X0 = torch.from_numpy(np.array(BR.x0(K))).to(gpu)
    Xw, itw, relw = BR.pcg_solve(K, kind, tol, 200, True)
    X, its, rel = pcg.solve(B, X0, tol=tol, max_iters=200, check_every=3, graph=True)
    assert itw <= its < itw + 6 and its % 3 == 0 and (rel <= tol * tol).all()
    X, its, rel = pcg.solve(B, X0, tol=tol, max_iters=200)
    assert its == itw < 200 and same_bits(rel, relw) and same_bits(X.cpu().numpy(), Xw)
    assert pcg.solve(B, max_iters=2)[1] == 2


def test_pcg_captured(gpu):
    """iterate(4) captured once (global capture mode: a hidden allocation,
    synchronisation or null-stream launch is an error) and replayed after
    start() on two right-hand sides equals the eager bits."""
    K, kind = 32, "multicolor"
    pcg = make_pcg(gpu, K, kind)
    B = torch.full((900, K), NAN, dtype=torch.float64, device=gpu)
    pcg.start(B)
    torch.cuda.synchronize()
    g, side = capture(lambda s: pcg.iterate(4, s))
    torch.cuda.synchronize()
    assert bool((pcg.X == 0).all()), "the capture executed"  # an iteration on the NaN B would have made X NaN
    for zero_col in (None, 4):
        B.copy_(torch.from_numpy(np.array(BR.rhs(K, zero_col))))
        pcg.start(B)
        g.replay()
        assert same_state(state(pcg), BR.pcg_iterations(K, kind, 4, False, zero_col)), zero_col
    del g


def test_pcg_stream_order(gpu):
    """start and iterate(4) eagerly on a side stream, no device-wide sync."""
    K, kind = 32, "multicolor"
    pcg = make_pcg(gpu, K, kind)
    Bsrc = torch.from_numpy(np.array(BR.rhs(K))).to(gpu)
    B = torch.full((900, K), NAN, dtype=torch.float64, device=gpu)

    def steps(s):
        pcg.start(B, stream=s)
        pcg.iterate(4, s)
    Xout = in_stream_order(torch.cuda.Stream(), B, Bsrc, steps, pcg.X, gpu)
    torch.cuda.synchronize()
    assert same_bits(Xout.cpu().numpy(), BR.pcg_iterations(K, kind, 4)["X"])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_python_refusals(gpu):
    m, K = 65, 8
    X = torch.zeros((m, K), dtype=torch.float64, device=gpu)
    v = torch.ones(K, dtype=torch.float64, device=gpu)
    bad = ((torch.zeros((m, K), device=gpu), TypeError),                       # float32
           (torch.zeros((m, K), dtype=torch.float64), TypeError),              # on the host
           (torch.zeros((m + 1, K), dtype=torch.float64, device=gpu), ValueError),
           (torch.zeros((m, K + 1), dtype=torch.float64, device=gpu), ValueError),
           (torch.zeros((K, m), dtype=torch.float64, device=gpu).t(), ValueError))  # not row-major
    for T, exc in bad:
        for call in (lambda: smfv.coldot(X, T), lambda: smfv.col_axpy(v, None, X, T), lambda: smfv.col_xpay(v, v, X, T),
                     lambda: smfv.pcg_update(v, v, X.clone(), X.clone(), X.clone(), T)):
            with pytest.raises(exc):
                call()
    for call in (lambda: smfv.col_axpy(v[:-1], None, X, X), lambda: smfv.col_axpy(v, torch.ones(2 * K, dtype=torch.float64, device=gpu)[::2], X, X),
                 lambda: smfv.coldot(X, X, out=v[:-1]), lambda: smfv.coldot(X, X, workspace=v[:1])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        smfv.col_axpy(v.cpu(), None, X, X)
    with pytest.raises(SmfvError, match="overlap"):
        smfv.pcg_update(v, v, X, X.clone(), X.clone(), X)  # P is R
    W = torch.zeros((m, 2 * K), dtype=torch.float64, device=gpu)
    with pytest.raises(SmfvError, match="overlap"):
        smfv.pcg_update(v, v, X, X.clone(), W[:, :K], W[:, K - 1:2 * K - 1])  # X and R share a column
    smfv.pcg_update(v, v, X, X.clone(), W[:, :K], W[:, K:])  # disjoint windows of one buffer are fine
    dA = csr_of(BR.laplacian(), gpu)
    with pytest.raises(ValueError):
        smfv.BlockPCG(smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, transpose=True), K)
    with pytest.raises(ValueError):
        smfv.BlockPCG(smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K), K + 1)
    with pytest.raises(TypeError):
        smfv.BlockPCG(dA, K, M=object())
    with pytest.raises(ValueError):
        smfv.BlockPCG(dA, K).start(torch.zeros((m, K), dtype=torch.float64, device=gpu))
    torch.cuda.synchronize()
