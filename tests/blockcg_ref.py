"""The independent reference for the coupled-block tests.

Plain numpy (no GPU, no torch, nothing from the library), built on the
references that already exist: the Gram rule is blockvec_ref.coldot column pair
by column pair, the small solve is ilu0_ref.factor followed by trsm_ref.solve
(lower with a unit diagonal, then upper) on the dense matrix written as CSR
with sorted columns, A P is the row-sequential loop of tests/adversarial.py.
The block . matrix rule is restated here, vectorised and as a plain triple
loop.  A coupled block PCG (O'Leary) is built from them in the exact sequence
of CoupledBlockPCG, and a column-wise PCG from blockvec_ref's pieces on the
same inputs.  Inputs and references are computed once and handed out
read-only.
"""
import functools

import numpy as np

import adversarial as adv
import blockvec_ref as BR
import ilu0_ref as I
import reorder_ref as R
import trsm_ref as T

_frozen = T._frozen
SHIFT = 0.01  # the solver's matrix: blockvec_ref.laplacian(30, SHIFT)


def gram(X, Y):
    """G[i, j] = coldot(X[:, i], Y[:, j]): row i is the column-dot rule on
    column i of X broadcast against Y."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    Ky = Y.shape[1]
    return np.stack([BR.coldot(np.repeat(X[:, i:i + 1], Ky, axis=1), Y) for i in range(X.shape[1])])


def block_mul(X, C, Z=None, negate=False):
    """Y = Z +- X C: acc = Z (or +0.0), then one rounded product and one
    rounded sum per l, ascending."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    c = -C if negate else C
    acc = np.zeros((X.shape[0], C.shape[1])) if Z is None else np.array(Z, np.float64)
    with np.errstate(all="ignore"):
        for l in range(X.shape[1]):
            acc = acc + X[:, l:l + 1] * c[l][None, :]
    return acc


def block_mul_loops(X, C, Z=None, negate=False):
    """The rule as the plain loops of its statement (small inputs only)."""
    m, Kx = X.shape
    Ky = C.shape[1]
    Y = np.empty((m, Ky))
    with np.errstate(all="ignore"):
        for i in range(m):
            for j in range(Ky):
                acc = np.float64(0.0) if Z is None else np.float64(Z[i, j])
                for l in range(Kx):
                    c = -np.float64(C[l, j]) if negate else np.float64(C[l, j])
                    acc = acc + np.float64(X[i, l]) * c
                Y[i, j] = acc
    return Y


def dense_csr(G):
    """The dense K x K matrix as CSR, every entry stored, columns sorted."""
    G = np.asarray(G, np.float64)
    K = G.shape[0]
    return adv.Csr(G.reshape(-1).copy(), np.tile(np.arange(K, dtype=np.int32), K),
                   (np.arange(K + 1) * K).astype(np.int32), K, K)


def lu(G):
    """ilu0_ref.factor on the dense CSR: LU without pivoting, as a CSR of factors."""
    A = dense_csr(G)
    return adv.Csr(I.factor(A), A.colIndices, A.rowPtr, A.numRows, A.numCols)


def small_solve(G, H, F=None):
    """C = G^-1 H: the factorisation, the lower solve with a unit diagonal, the upper solve."""
    F = lu(G) if F is None else F
    return T.solve(F, T.solve(F, np.asarray(H, np.float64), True, True), False, False)


# ---------------------------------------------------------------------------
# small systems: well conditioned without pivoting, and the special values
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def system(K):
    """(G, H[K x 128], F): G random with a dominant diagonal of mixed sign."""
    rng = np.random.default_rng(4000 + K)
    G = rng.uniform(-1, 1, (K, K))
    d = 1.0 + np.abs(G).sum(1)
    G[np.arange(K), np.arange(K)] = np.where(np.arange(K) % 3 == 0, -d, d)
    H = rng.uniform(-1, 1, (K, 128))
    return _frozen(G), _frozen(H), lu(G)


@functools.lru_cache(None)
def solution(K, N):
    G, H, F = system(K)
    return _frozen(small_solve(G, H[:, :N], F))


@functools.lru_cache(None)
def special_systems():
    """name -> (G, H, C): a pivot cancelling to exactly +0.0, NaN, +-inf and
    -0.0 in G and H."""
    out = {}
    rng = np.random.default_rng(41)
    base = rng.uniform(-1, 1, (8, 8)) + 6.0 * np.eye(8)
    H = rng.uniform(-1, 1, (8, 5))
    G = base.copy()
    G[0, 0], G[0, 1], G[1, 0], G[1, 1] = 2.0, 3.0, 4.0, 6.0  # W[1,1] = 6 - (4/2) * 3 = +0.0
    out["zero_pivot"] = (G, H)
    G = base.copy()
    G[3, 4] = np.nan
    out["nan"] = (G, H)
    G = base.copy()
    G[2, 5], G[6, 1] = np.inf, -np.inf
    out["inf"] = (G, H)
    G, H2 = base.copy(), H.copy()
    G[1, 0], G[0, 3], G[5, 7] = -0.0, -0.0, 0.0
    H2[0, :], H2[4, 2] = -0.0, -0.0
    out["neg_zero"] = (G, H2)
    H3 = H.copy()
    H3[2, 1], H3[7, 3], H3[0, 4] = np.nan, np.inf, -np.inf
    out["rhs_special"] = (base.copy(), H3)
    return {k: (_frozen(g), _frozen(h), _frozen(small_solve(g, h))) for k, (g, h) in out.items()}


# ---------------------------------------------------------------------------
# the solvers: coupled block PCG, and column-wise PCG on the same inputs
# ---------------------------------------------------------------------------
def matrix():
    return BR.laplacian(30, SHIFT)


@functools.lru_cache(None)
def rhs(K, dup=False):
    """blockvec_ref's right-hand sides (the matrix has as many rows); dup:
    column 1 repeats column 0, a rank-deficient block."""
    B = np.array(BR.rhs(K))
    if dup:
        B[:, 1] = B[:, 0]
    return _frozen(B)


@functools.lru_cache(None)
def preconditioner(kind):
    """None, or a function Z = M(R) by the reference factorisation and solves."""
    A = matrix()
    if kind is None:
        return None
    if kind == "natural":
        F = adv.Csr(I.factor(A), A.colIndices, A.rowPtr, A.numRows, A.numCols)
        return lambda Rm: T.solve(F, T.solve(F, Rm, True, True), False, False)
    assert kind == "multicolor"
    perm, _, _ = R.multicolor(A)
    Bm, _ = R.permute(A, perm)
    F = adv.Csr(I.factor(Bm), Bm.colIndices, Bm.rowPtr, Bm.numRows, Bm.numCols)

    def apply(Rm):
        Z = T.solve(F, T.solve(F, Rm[perm], True, True), False, False)
        out = np.empty_like(Z)
        out[perm] = Z
        return out
    return apply


def _start(B, X0, M):
    A = matrix()
    if X0 is None:
        X, Rm = np.zeros_like(B), np.array(B)
    else:
        X = np.array(X0)
        Rm = B - adv.ref_f64(A, X)
    Z = Rm if M is None else M(Rm)
    return dict(X=X, R=Rm, Z=Z, P=np.array(Z), rho=gram(Z, Rm), bb=BR.coldot(B, B), rr=None)


def _iterate(st, M):
    A = matrix()
    with np.errstate(all="ignore"):
        Q = adv.ref_f64(A, st["P"])
        alpha = small_solve(gram(st["P"], Q), st["rho"])
        st["X"] = block_mul(st["P"], alpha, st["X"])
        st["R"] = block_mul(Q, alpha, st["R"], negate=True)
        st["Z"] = st["R"] if M is None else M(st["R"])
        rho_new = gram(st["Z"], st["R"])
        st["rr"] = np.diag(rho_new).copy() if M is None else BR.coldot(st["R"], st["R"])
        beta = small_solve(st["rho"], rho_new)
        st["P"] = block_mul(st["P"], beta, st["Z"])
        st["rho"] = rho_new


@functools.lru_cache(None)
def iterations(K, kind, n, with_x0=False):
    """The state (X, R, P, rho, rr, bb) after n iterations, read-only."""
    M = preconditioner(kind)
    st = _start(rhs(K), BR.x0(K) if with_x0 else None, M)
    for _ in range(n):
        _iterate(st, M)
    return {k: (_frozen(np.array(v)) if v is not None else None) for k, v in st.items()}


@functools.lru_cache(None)
def solve(K, kind, tol, max_iters, dup=False):
    """(X, iterations, rr / bb, breakdown) of CoupledBlockPCG.solve with
    check_every = 1: stop when every rr[j] <= tol^2 bb[j], or at the first
    non-finite rr (breakdown)."""
    M = preconditioner(kind)
    st = _start(rhs(K, dup), None, M)
    it, broke = 0, False
    while it < max_iters:
        _iterate(st, M)
        it += 1
        if not np.all(np.isfinite(st["rr"])):
            broke = True
            break
        if np.all(st["rr"] <= (tol * tol) * st["bb"]):
            break
    return _frozen(st["X"]), it, _frozen(BR.relative(st["rr"], st["bb"])), broke


@functools.lru_cache(None)
def columnwise_solve(K, tol, max_iters):
    """blockvec_ref's column-wise loop (BlockPCG's sequence, M = None) on this
    file's matrix and right-hand sides: (X, iterations)."""
    A, B = matrix(), rhs(K)
    X, Rm = np.zeros_like(B), np.array(B)
    P, rz, bb = np.array(Rm), BR.coldot(Rm, Rm), BR.coldot(B, B)
    it = 0
    while it < max_iters:
        Q = adv.ref_f64(A, P)
        X, Rm, rr = BR.pcg_update(rz, BR.coldot(P, Q), BR.ZERO_DEN, P, Q, X, Rm)
        P = BR.xpay(rr, rz, BR.ZERO_DEN, Rm, P)
        rz = rr
        it += 1
        if np.all(rr <= (tol * tol) * bb):
            break
    return _frozen(X), it


def true_relative_residual(X, K):
    """||B - A X|| / ||B|| per column, in plain numpy."""
    B = rhs(K)
    Rm = B - adv.ref_f64(matrix(), X)
    return np.sqrt((Rm * Rm).sum(0) / (B * B).sum(0))
