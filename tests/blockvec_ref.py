"""The independent reference for the block-vector tests.

Plain numpy (no GPU, no torch, nothing from the library): the column-dot rule
of include/smfv.h in vectorised form (coldot) and as a plain triple loop
(coldot_loops), the scalar rule, axpy / xpay, and a PCG loop built from them
in the exact sequence of BlockPCG, with A P by the row-sequential loop of
tests/adversarial.py and M from ilu0_ref, trsm_ref and reorder_ref.  Inputs
and references are computed once and handed out read-only.
"""
import functools

import numpy as np

import adversarial as adv
import ilu0_ref as I
import reorder_ref as R
import trsm_ref as T

CHUNK, STRANDS = 512, 32  # the two constants of the rule (pinned by test_blockvec_host.py)
NEGATE, ZERO_DEN = 1, 2   # SMFV_COL_NEGATE, SMFV_COL_ZERO_DEN
_frozen = T._frozen


def coldot(X, Y):
    """The rule, vectorised: zero-pad to whole chunks (a missing row is a
    product of +0.0 and an accumulator that starts at +0.0 never becomes
    -0.0), strands by reshape, ascending t, the tree, the chunks in order."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    m, K = X.shape
    nch = -(-m // CHUNK)
    with np.errstate(all="ignore"):
        prod = np.zeros((nch * CHUNK, K))
        prod[:m] = X * Y
        prod = prod.reshape(nch, CHUNK // STRANDS, STRANDS, K)  # [chunk, t, strand, column]
        v = np.zeros((nch, STRANDS, K))
        for t in range(CHUNK // STRANDS):
            v = v + prod[:, t]
        h = STRANDS // 2
        while h >= 1:
            v = v[:, :h] + v[:, h:2 * h]
            h //= 2
        d = np.zeros(K)
        for c in range(nch):
            d = d + v[c, 0]
    return d


def coldot_loops(X, Y):
    """The rule as the plain loops of its statement (small inputs only)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    m, K = X.shape
    out = np.zeros(K)
    with np.errstate(all="ignore"):
        for j in range(K):
            d = np.float64(0.0)
            for c0 in range(0, m, CHUNK):
                end = min(m, c0 + CHUNK)
                v = []
                for s in range(STRANDS):
                    a = np.float64(0.0)
                    for r in range(c0 + s, end, STRANDS):
                        a = a + X[r, j] * Y[r, j]
                    v.append(a)
                h = STRANDS // 2
                while h >= 1:
                    for s in range(h):
                        v[s] = v[s] + v[s + h]
                    h //= 2
                d = d + v[0]
            out[j] = d
    return out


def rowseq_dot(X, Y):
    """What the rule is NOT: one accumulator per column over the rows in order."""
    d = np.zeros(X.shape[1])
    with np.errstate(all="ignore"):
        for r in range(X.shape[0]):
            d = d + X[r] * Y[r]
    return d


def scalar(num, den, flags):
    """s[j] of the scalar rule."""
    num = np.asarray(num, np.float64)
    with np.errstate(all="ignore"):
        if den is None:
            s = num.copy()
        else:
            den = np.asarray(den, np.float64)
            s = num / den
            if flags & ZERO_DEN:
                s = np.where(den == 0.0, 0.0, s)
        if flags & NEGATE:
            s = -s
    return s


def axpy(num, den, flags, X, Y):
    with np.errstate(all="ignore"):
        return Y + scalar(num, den, flags)[None, :] * X


def xpay(num, den, flags, X, Y):
    with np.errstate(all="ignore"):
        return X + scalar(num, den, flags)[None, :] * Y


def pcg_update(num, den, flags, P, Q, X, R):
    """(X', R', rr) of the fused update: the three separate rules."""
    Xn = axpy(num, den, flags, P, X)
    Rn = axpy(num, den, flags ^ NEGATE, Q, R)
    return Xn, Rn, coldot(Rn, Rn)


# ---------------------------------------------------------------------------
# the PCG problem: a 30 x 30 five-point Laplacian plus a diagonal shift
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def laplacian(n=30, shift=1.0):
    rows_c, rows_v = [], []
    for y in range(n):
        for x in range(n):
            c, v = [], []
            for dy, dx in ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)):
                yy, xx = y + dy, x + dx
                if 0 <= yy < n and 0 <= xx < n:
                    c.append(yy * n + xx)
                    v.append(4.0 + shift if (dy, dx) == (0, 0) else -1.0)
            rows_c.append(c)
            rows_v.append(v)
    rp = np.zeros(n * n + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows_c])
    A = adv.Csr(np.array(sum(rows_v, []), np.float64), np.array(sum(rows_c, []), np.int32), rp, n * n, n * n)
    return T.freeze(A)


@functools.lru_cache(None)
def rhs(K, zero_col=None):
    B = np.random.default_rng(900 + K).uniform(-1, 1, (laplacian().numRows, K))
    if zero_col is not None:
        B[:, zero_col] = 0.0
    return _frozen(B)


@functools.lru_cache(None)
def x0(K):
    return _frozen(np.random.default_rng(77 + K).uniform(-1, 1, (laplacian().numRows, K)))


@functools.lru_cache(None)
def _preconditioner(kind):
    """None, or a function Z = M(R) by the reference factorisation and solves."""
    A = laplacian()
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
    A = laplacian()
    if X0 is None:
        X, Rm = np.zeros_like(B), np.array(B)
    else:
        X = np.array(X0)
        Rm = B - adv.ref_f64(A, X)
    Z = Rm if M is None else M(Rm)
    return dict(X=X, R=Rm, Z=Z, P=np.array(Z), rz=coldot(Rm, Z), bb=coldot(B, B), rr=None)


def _iterate(st, M):
    A = laplacian()
    Q = adv.ref_f64(A, st["P"])
    pq = coldot(st["P"], Q)
    st["X"], st["R"], st["rr"] = pcg_update(st["rz"], pq, ZERO_DEN, st["P"], Q, st["X"], st["R"])
    st["Z"] = st["R"] if M is None else M(st["R"])
    rz_new = st["rr"] if M is None else coldot(st["R"], st["Z"])
    st["P"] = xpay(rz_new, st["rz"], ZERO_DEN, st["Z"], st["P"])
    st["rz"] = rz_new


@functools.lru_cache(None)
def pcg_iterations(K, kind, n, with_x0=False, zero_col=None):
    """The state (X, R, P, rr, bb) after n iterations, read-only."""
    M = _preconditioner(kind)
    st = _start(rhs(K, zero_col), x0(K) if with_x0 else None, M)
    for _ in range(n):
        _iterate(st, M)
    return {k: (_frozen(np.array(v)) if v is not None else None) for k, v in st.items()}


@functools.lru_cache(None)
def pcg_solve(K, kind, tol, max_iters, with_x0=False, zero_col=None):
    """(X, iterations, rr / bb) of BlockPCG.solve with check_every = 1: column
    j has converged when rr[j] <= (tol * tol) * bb[j]; all columns iterate
    until all have."""
    M = _preconditioner(kind)
    st = _start(rhs(K, zero_col), x0(K) if with_x0 else None, M)
    it = 0
    while it < max_iters:
        _iterate(st, M)
        it += 1
        if np.all(st["rr"] <= (tol * tol) * st["bb"]):
            break
    return _frozen(st["X"]), it, _frozen(relative(st["rr"], st["bb"]))


def relative(rr, bb):
    """rr / bb per column; 0 for a zero right-hand side met exactly."""
    with np.errstate(all="ignore"):
        return np.where(bb == 0.0, np.where(rr == 0.0, 0.0, np.inf), rr / bb)
