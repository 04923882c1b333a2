"""The coupled-block family on the GPU (smfv_gram_f64, smfv_block_mul_f64,
smfv_small_solve_f64, CoupledBlockPCG): every comparison is bit for bit through
an int64 view against the numpy references of tests/blockcg_ref.py (never the
library); where a NaN is the expected result only its position is compared.
"""
import numpy as np
import pytest
import torch

import blockcg_ref as CR
import blockvec_ref as BR
from test_gpu_blockvec import GUARD, Window, band_ok, bits, cols, same_bits, uniform
from test_gpu_capture import NAN, capture, in_stream_order
from test_gpu_reorder import BIG_F, BIG_LD, BIG_M, big_buffer, csr_of  # noqa: F401  (big_buffer is a fixture)

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import engine
from sparsematrixmultiplicationmpi_amd._lib import SmfvError

pytestmark = pytest.mark.gpu
MS = [0, 1, 31, 32, 33, 511, 512, 513, 1025, 1500]  # a strand edge, a chunk edge, a short last chunk, three chunks
KK = [(1, 1), (3, 8), (32, 32), (33, 31), (128, 5), (64, 64), (128, 128), (40, 40)]
SOLVE_K = [1, 2, 3, 8, 31, 32, 33, 64, 128]
VIEWS = ((0, 0, 0, 0), (6, 2, 3, 0), (3, 5, 2, 0), (2, 2, 1, 1))  # padding of X, Y / Z, the output; doubles off alignment


@pytest.fixture(autouse=True)
def _tiling_reset():
    yield
    engine.gram_set_tiling(0)


def run_gram(Xh, Yh, gpu, px, py, pg, shift, x_is_y=False):
    """gram with X, Y, G and a NaN-prefilled workspace as windows of NaN-filled
    buffers; the guards, the padding and the inputs are checked."""
    (m, Kx), Ky = Xh.shape, Yh.shape[1]
    X = Window(Xh, Kx + px, shift, gpu)
    Y = X if x_is_y else Window(Yh, Ky + py, shift, gpu)
    G = Window(np.full((Kx, Ky), NAN), Ky + pg, shift, gpu)
    wbuf, ws = cols(np.full(smfv.gram_workspace_doubles(m, Kx, Ky), NAN), gpu)
    got = smfv.gram(X.v, Y.v, out=G.v, workspace=ws)
    assert got is G.v
    torch.cuda.synchronize()
    assert band_ok(wbuf, ws), "written outside the workspace"
    assert same_bits(X.read(), Xh) and same_bits(Y.read(), Yh), "an input changed"
    return G.read()


# ---------------------------------------------------------------------------
# gram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Kx,Ky", KK)
@pytest.mark.parametrize("m", MS)
def test_gram(gpu, m, Kx, Ky):
    """Against blockvec_ref.coldot column pair by column pair: contiguous
    (16-byte loads at even widths), padded leading dimensions, views one double
    off alignment, every register tiling, X is Y; the workspace starts as NaN,
    the band around G stays NaN; no entry is -0.0, m = 0 gives +0.0."""
    X, Y = uniform(m, Kx, 1000 * m + Kx), uniform(m, Ky, 1000 * m + Ky + 500)
    want = CR.gram(X, Y)
    for px, py, pg, shift in VIEWS:
        got = run_gram(X, Y, gpu, px, py, pg, shift)
        assert same_bits(got, want), (px, py, pg, shift)
        assert not (np.signbit(got) & (got == 0)).any()  # never -0.0
    for tiling in (1, 2, 3):
        engine.gram_set_tiling(tiling)
        assert same_bits(run_gram(X, Y, gpu, 0, 0, 0, 0), want), tiling
        assert same_bits(run_gram(X, Y, gpu, 1, 3, 2, 1), want), tiling
    engine.gram_set_tiling(0)
    if m == 0:
        assert np.array_equal(bits(got), np.zeros((Kx, Ky), np.int64))  # +0.0
    if Kx == Ky:
        got = run_gram(X, X, gpu, 2, 2, 0, 0, x_is_y=True)
        assert same_bits(got, CR.gram(X, X))


@pytest.mark.parametrize("m,K", [(1025, 32), (700, 33), (1500, 5)])
def test_gram_against_device_coldot(gpu, m, K):
    """Row i of G equals the device coldot of column i broadcast against Y,
    and diag(gram(R, R)) == coldot(R, R), on the device alone."""
    X, Y = (torch.from_numpy(uniform(m, K, 5 * m + K + i)).to(gpu) for i in range(2))
    G = smfv.gram(X, Y).cpu().numpy()
    for i in (0, K // 2, K - 1):
        row = smfv.coldot(X[:, i:i + 1].expand(m, K).contiguous(), Y).cpu().numpy()
        assert same_bits(G[i], row), i
    assert same_bits(np.diag(smfv.gram(X, X).cpu().numpy()), smfv.coldot(X, X).cpu().numpy())


def test_gram_special_values(gpu):
    """NaN, +-inf, inf * 0, inf - inf across strands and chunks, subnormal
    products, 2^+-600, columns cancelling to +0.0 and of -0.0 products: the
    block-vector special block crossed with itself, every tiling."""
    from test_gpu_blockvec import special_blocks
    X, Y = special_blocks()
    want = CR.gram(X, Y)
    assert np.isnan(want).any() and np.isinf(want).any() and same_bits(np.diag(want), BR.coldot(X, Y))
    for tiling in (0, 1, 2, 3):
        engine.gram_set_tiling(tiling)
        for px, py, pg, shift in ((0, 0, 0, 0), (1, 1, 1, 1)):
            got = run_gram(X, Y, gpu, px, py, pg, shift)
            assert same_bits(got, want), (tiling, shift)
            assert not (np.signbit(got) & (got == 0)).any()


# ---------------------------------------------------------------------------
# block_mul
# ---------------------------------------------------------------------------
def special_mul(m, Kx, Ky, seed):
    """X, C, Z with NaN, +-inf, -0.0, subnormals and 2^+-600 in places."""
    X, C, Z = uniform(m, Kx, seed), uniform(Kx, Ky, seed + 1), uniform(m, Ky, seed + 2)
    if m >= 31 and Kx >= 3:
        X[0, 1], X[3, 0], X[5, Kx - 1] = np.nan, np.inf, 2.0 ** 600
        X[7, :], Z[7, :] = -0.0, -0.0
        X[9, :] *= 1e-160
        C[2, 0], C[1, Ky - 1] = -np.inf, 2.0 ** -600
        C[0, Ky // 2] = -0.0
        Z[11, 0] = np.nan
    return X, C, Z


@pytest.mark.parametrize("Kx,Ky", KK)
@pytest.mark.parametrize("m", MS)
def test_block_mul(gpu, m, Kx, Ky):
    """Against the numpy rule: Z given, Z None, Y == Z, negate, padded and
    misaligned windows (padding and guards still NaN, X, C and Z unchanged),
    Y == X where Kx == Ky, special values."""
    X, C, Z = special_mul(m, Kx, Ky, 17 * m + Kx + Ky)
    for v, (px, pz, py, shift) in enumerate(VIEWS):
        neg = bool(v & 1)
        wx, wc, wz = Window(X, Kx + px, shift, gpu), Window(C, Ky + py, shift, gpu), Window(Z, Ky + pz, shift, gpu)
        wy = Window(np.full((m, Ky), NAN), Ky + py, shift, gpu)
        out = smfv.block_mul(wx.v, wc.v, wz.v, wy.v, negate=neg)
        assert out is wy.v
        torch.cuda.synchronize()
        assert same_bits(wy.read(), CR.block_mul(X, C, Z, neg)), (px, pz, py, shift)
        smfv.block_mul(wx.v, wc.v, None, wy.v, negate=not neg)
        smfv.block_mul(wx.v, wc.v, wz.v, wz.v, negate=neg)  # Y is Z
        torch.cuda.synchronize()
        assert same_bits(wy.read(), CR.block_mul(X, C, None, not neg)), (px, pz, py, shift)
        assert same_bits(wz.read(), CR.block_mul(X, C, Z, neg)), (px, pz, py, shift)
        assert same_bits(wx.read(), X) and same_bits(wc.read(), C)
        if Kx == Ky:  # Y is X, Z apart and Z None
            wz = Window(Z, Ky + pz, shift, gpu)
            smfv.block_mul(wx.v, wc.v, wz.v, wx.v, negate=neg)
            torch.cuda.synchronize()
            assert same_bits(wx.read(), CR.block_mul(X, C, Z, neg)) and same_bits(wz.read(), Z), (px, shift)
            wx = Window(X, Kx + px, shift, gpu)
            smfv.block_mul(wx.v, wc.v, None, wx.v)
            torch.cuda.synchronize()
            assert same_bits(wx.read(), CR.block_mul(X, C))


@pytest.mark.parametrize("m,K", [(9000, 128), (110_000, 32)])
def test_block_mul_many_batches(gpu, m, K):
    """More row batches than resident blocks: a block walks several batches
    against one copy of C.  In place (Y == X == P), as the solver calls it."""
    X, C, Z = uniform(m, K, m), uniform(K, K, m + 1), uniform(m, K, m + 2)
    dX, dC, dZ = (torch.from_numpy(a).to(gpu) for a in (X, C, Z))
    smfv.block_mul(dX, dC, dZ, dX)
    assert same_bits(dX.cpu().numpy(), CR.block_mul(X, C, Z))
    assert same_bits(dZ.cpu().numpy(), Z)


# ---------------------------------------------------------------------------
# small_solve
# ---------------------------------------------------------------------------
def run_solve(G, H, gpu, pad, shift, in_place):
    K, N = H.shape
    wg, wh = Window(G, K + pad, shift, gpu), Window(H, N + pad, shift, gpu)
    wc = wh if in_place else Window(np.full((K, N), NAN), N + 2 * pad, shift, gpu)
    out = smfv.small_solve(wg.v, wh.v, wc.v)
    assert out is wc.v
    torch.cuda.synchronize()
    assert same_bits(wg.read(), G) and (in_place or same_bits(wh.read(), H)), "an input changed"
    return wc.read()


@pytest.mark.parametrize("K", SOLVE_K)
def test_small_solve(gpu, K):
    """Against ilu0_ref.factor + trsm_ref.solve on the dense CSR, N in
    {1, K, 128} (K = 128 with N = 128 keeps T in C, the others in LDS):
    contiguous, padded and misaligned, C == H; G unchanged, the bands NaN."""
    G, H, _ = CR.system(K)
    for N in sorted({1, K, 128}):
        want = CR.solution(K, N)
        for pad, shift, in_place in ((0, 0, False), (3, 1, False), (2, 0, True), (1, 1, True)):
            assert same_bits(run_solve(G, H[:, :N], gpu, pad, shift, in_place), want), (N, pad, shift, in_place)


@pytest.mark.parametrize("name", ["zero_pivot", "nan", "inf", "neg_zero", "rhs_special"])
def test_small_solve_special_values(gpu, name):
    G, H, want = CR.special_systems()[name]
    assert same_bits(run_solve(G, H, gpu, 0, 0, False), want)
    assert same_bits(run_solve(G, H, gpu, 2, 1, True), want)


# ---------------------------------------------------------------------------
# rows beyond 4 GiB
# ---------------------------------------------------------------------------
def test_large_offsets(gpu, big_buffer):
    """A leading dimension of 8.95 million doubles: rows 60.. of a 70-row
    window lie beyond 4 GiB.  gram with X there, then with G there (Kx = 70);
    block_mul with X there, then with Y there; two guard columns on each side
    of an output still NaN."""
    K = 32
    assert 59 * BIG_LD * 8 < 1 << 32 <= 60 * BIG_LD * 8
    big = big_buffer.view(BIG_M, BIG_LD)
    wide, win = big[:, BIG_F - 2:BIG_F + K + 2], big[:, BIG_F:BIG_F + K]
    dev = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    A, B = uniform(BIG_M, K, 70), uniform(BIG_M, K, 71)
    win.copy_(dev(A))
    assert same_bits(smfv.gram(win, dev(B)).cpu().numpy(), CR.gram(A, B))
    X, Y = uniform(40, BIG_M, 72), uniform(40, K, 73)  # G is 70 x 32
    wide.fill_(NAN)
    smfv.gram(dev(X), dev(Y), out=win)
    h = wide.cpu().numpy()
    assert np.isnan(h[:, :2]).all() and np.isnan(h[:, -2:]).all(), "written outside G's window"
    assert same_bits(h[:, 2:-2], CR.gram(X, Y))
    C, Z = uniform(K, K, 74), uniform(BIG_M, K, 75)
    win.copy_(dev(A))
    assert same_bits(smfv.block_mul(win, dev(C), dev(Z)).cpu().numpy(), CR.block_mul(A, C, Z))
    wide.fill_(NAN)
    smfv.block_mul(dev(A), dev(C), dev(Z), win, negate=True)
    h = wide.cpu().numpy()
    assert np.isnan(h[:, :2]).all() and np.isnan(h[:, -2:]).all(), "written outside Y's window"
    assert same_bits(h[:, 2:-2], CR.block_mul(A, C, Z, True))


# ---------------------------------------------------------------------------
# CoupledBlockPCG
# ---------------------------------------------------------------------------
def make_pcg(gpu, K, kind):
    dA = csr_of(CR.matrix(), gpu)
    M = None if kind is None else smfv.Ilu0Preconditioner(dA, K, reorder=None if kind == "natural" else "multicolor")
    return smfv.CoupledBlockPCG(dA, K, M)


def state(pcg):
    torch.cuda.synchronize()
    st = {k: getattr(pcg, k).cpu().numpy() for k in ("X", "R", "P", "rr")}
    st["rho"] = pcg._rho(pcg._par).cpu().numpy()
    return st


def same_state(got, want):
    return all(same_bits(got[k], want[k]) for k in ("X", "R", "P", "rr", "rho"))


@pytest.mark.parametrize("kind", [None, "natural", "multicolor"])
@pytest.mark.parametrize("K", [3, 8, 32])
def test_pcg_iterations(gpu, K, kind):
    """X, R, P, rho and rr after 1, 2 and 5 iterations equal the numpy loop bit
    for bit; with X0 given too."""
    pcg = make_pcg(gpu, K, kind)
    B = torch.from_numpy(np.array(CR.rhs(K))).to(gpu)
    pcg.start(B)
    for n, total in ((1, 1), (1, 2), (3, 5)):
        pcg.iterate(n)
        assert same_state(state(pcg), CR.iterations(K, kind, total)), total
    want = CR.iterations(K, kind, 5)
    assert same_bits(pcg.bb.cpu().numpy(), want["bb"]) and pcg.iterations == 5
    assert np.isfinite(want["X"]).all() and want["rr"].max() < want["bb"].min()  # it is converging
    pcg.start(B, torch.from_numpy(np.array(BR.x0(K))).to(gpu))
    pcg.iterate(2)
    pcg.iterate(3)
    assert same_state(state(pcg), CR.iterations(K, kind, 5, True))


@pytest.mark.parametrize("kind", [None, "multicolor"])
def test_pcg_solve(gpu, kind):
    """solve: the iteration count, X and rr / bb equal the numpy loop's;
    without M at most half BlockPCG's count; a captured solve equals the
    launched one; residuals() is (rr, bb)."""
    K, tol = 32, 1e-8
    pcg = make_pcg(gpu, K, kind)
    B = torch.from_numpy(np.array(CR.rhs(K))).to(gpu)
    X, its, rel = pcg.solve(B, tol=tol, max_iters=200)
    Xw, itw, relw, broke = CR.solve(K, kind, tol, 200)
    Xh = X.cpu().numpy()
    assert not broke and not pcg.breakdown
    assert its == itw and 3 < its < 200 and same_bits(rel, relw) and same_bits(Xh, Xw)
    assert (rel <= tol * tol).all()
    if kind is None:
        assert 2 * its <= CR.columnwise_solve(K, tol, 200)[1]
    rr, bb = pcg.residuals()
    assert same_bits(rr, pcg.rr.cpu().numpy()) and same_bits(bb, pcg.bb.cpu().numpy()) and same_bits(BR.relative(rr, bb), rel)
    Xg, itg, relg = pcg.solve(B, tol=tol, max_iters=200, graph=True)
    assert itg == its and same_bits(relg, rel) and same_bits(Xg.cpu().numpy(), Xh)
    X, its3, rel3 = pcg.solve(B, tol=tol, max_iters=200, check_every=3, graph=True)
    assert its <= its3 < its + 3 and its3 % 3 == 0
    assert pcg.solve(B, max_iters=2)[1] == 2


def test_pcg_breakdown(gpu):
    """Two identical right-hand-side columns: Gamma is singular, the pivot
    cancels to exactly zero, NaN spreads; solve stops at the first check, sets
    breakdown and returns, where the numpy loop stops too."""
    K = 8
    pcg = make_pcg(gpu, K, None)
    B = torch.from_numpy(np.array(CR.rhs(K, True))).to(gpu)
    X, its, rel = pcg.solve(B, max_iters=50)
    _, itw, relw, broke = CR.solve(K, None, 1e-8, 50, True)
    assert broke and pcg.breakdown and its == itw < 50 and same_bits(rel, relw)
    assert not np.isfinite(rel).all()
    pcg.solve(torch.from_numpy(np.array(CR.rhs(K))).to(gpu), max_iters=3)
    assert not pcg.breakdown  # start() clears it


def test_pcg_captured(gpu):
    """iterate(2) captured once (global capture mode: a hidden allocation,
    synchronisation or null-stream launch is an error) and replayed twice
    after start() equals four eager iterations."""
    K, kind = 32, "multicolor"
    pcg = make_pcg(gpu, K, kind)
    B = torch.full((900, K), NAN, dtype=torch.float64, device=gpu)
    pcg.start(B)
    torch.cuda.synchronize()
    g, side = capture(lambda s: pcg.iterate(2, s))
    torch.cuda.synchronize()
    assert bool((pcg.X == 0).all()), "the capture executed"  # an iteration on the NaN B would have made X NaN
    B.copy_(torch.from_numpy(np.array(CR.rhs(K))))
    pcg.start(B)
    g.replay()
    assert same_state(state(pcg), CR.iterations(K, kind, 2))
    g.replay()
    assert same_state(state(pcg), CR.iterations(K, kind, 4))
    del g


def test_pcg_stream_order(gpu):
    """start and iterate(3) eagerly on a side stream, no device-wide sync."""
    K, kind = 32, "multicolor"
    pcg = make_pcg(gpu, K, kind)
    Bsrc = torch.from_numpy(np.array(CR.rhs(K))).to(gpu)
    B = torch.full((900, K), NAN, dtype=torch.float64, device=gpu)

    def steps(s):
        pcg.start(B, stream=s)
        pcg.iterate(3, s)
    Xout = in_stream_order(torch.cuda.Stream(), B, Bsrc, steps, pcg.X, gpu)
    torch.cuda.synchronize()
    assert same_bits(Xout.cpu().numpy(), CR.iterations(K, kind, 3)["X"])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_python_refusals(gpu):
    m, K = 65, 8
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=gpu)  # noqa: E731
    X, C = new(m, K), new(K, K)
    bad = ((torch.zeros((m, K), device=gpu), TypeError),          # float32
           (torch.zeros((m, K), dtype=torch.float64), TypeError),  # on the host
           (new(m + 1, K), ValueError),
           (new(K, m).t(), ValueError))                            # not row-major
    for T, exc in bad:
        for call in (lambda: smfv.gram(X, T), lambda: smfv.block_mul(X, C, T), lambda: smfv.block_mul(X, C, None, T)):
            with pytest.raises(exc):
                call()
    for call in (lambda: smfv.gram(X, X, out=new(K, K + 1)), lambda: smfv.gram(X, X, workspace=new(3)),
                 lambda: smfv.block_mul(X, new(K + 1, K)), lambda: smfv.small_solve(new(K, K + 1), C),
                 lambda: smfv.small_solve(C, new(K + 1, 2)), lambda: smfv.small_solve(C, C, new(K, K + 1))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(SmfvError, match="Kx = 129"):
        smfv.gram(new(4, 129), new(4, 2))
    with pytest.raises(SmfvError, match="X and Y overlap"):
        smfv.block_mul(X, new(K, 5), None, X[:, :5])  # Y inside X, Kx != Ky
    W = new(m, 2 * K)
    with pytest.raises(SmfvError, match="X and Y overlap"):
        smfv.block_mul(W[:, :K], C, None, W[:, K - 1:2 * K - 1])  # sharing a column
    with pytest.raises(SmfvError, match="Z and Y overlap"):
        smfv.block_mul(X, C, W[:, :K], W[:, 1:K + 1])
    smfv.block_mul(W[:, :K], C, None, W[:, K:])  # disjoint windows of one buffer are fine
    with pytest.raises(SmfvError, match="G and C overlap"):
        smfv.small_solve(C, new(K, K), C)
    with pytest.raises(SmfvError, match="K = 129"):
        smfv.small_solve(new(129, 129), new(129, 1))
    dA = csr_of(CR.matrix(), gpu)
    with pytest.raises(ValueError):
        smfv.CoupledBlockPCG(smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, transpose=True), K)
    with pytest.raises(ValueError):
        smfv.CoupledBlockPCG(smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K), K + 1)
    with pytest.raises(ValueError):
        smfv.CoupledBlockPCG(dA, 129)
    with pytest.raises(TypeError):
        smfv.CoupledBlockPCG(dA, K, M=object())
    with pytest.raises(ValueError):
        smfv.CoupledBlockPCG(dA, K).start(new(m, K))
    torch.cuda.synchronize()
    assert GUARD == 16
