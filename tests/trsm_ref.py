"""Inputs and the independent reference for the triangular-solve tests.

Plain numpy (no GPU, no torch, nothing from the library): the sequential
substitution of include/smfv.h restated as a loop over each row's entries in
CSR order, vectorised over the K columns only (solve), the level of every row
(levels), and the test matrices: `band` (tests/adversarial.py's pattern with a
dominant, partly duplicated diagonal), `two_level`, the degenerate shapes and
the special-values case.  Every input and reference is computed once, shared
by the tests that need it and handed out read-only.
"""
import functools

import numpy as np

import adversarial as adv

M = 3000
KMAX = 128  # references are computed at K = 128; columns are independent, so K < 128 is a column slice


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def freeze(A):
    return adv.Csr(_frozen(A.values), _frozen(A.colIndices), _frozen(A.rowPtr), A.numRows, A.numCols)


def with_diag(A, seed):
    """Every row lacking a diagonal entry gets one, every 11th row a second
    one, the rows are reshuffled, and the diagonal total is +-(1 + sum |off-
    diagonal|) split unevenly over its duplicates."""
    rng = np.random.default_rng(seed)
    rows_c, rows_v = [], []
    for r in range(A.numRows):
        s, e = int(A.rowPtr[r]), int(A.rowPtr[r + 1])
        c = A.colIndices[s:e].astype(np.int64)
        v = A.values[s:e].copy()
        if not (c == r).any():
            c = np.append(c, r)
            v = np.append(v, 0.0)
        if r % 11 == 3:
            c = np.append(c, r)
            v = np.append(v, 0.0)
        o = rng.permutation(c.size)
        c, v = c[o], v[o]
        off = c != r
        tot = np.abs(v[off]).sum()
        dpos = np.flatnonzero(~off)
        sign = -1.0 if r % 5 == 0 else 1.0
        share = (1.0 + tot) / dpos.size
        v[dpos] = sign * share * (1 + 0.25 * rng.uniform(-1, 1, dpos.size))
        rows_c.append(c)
        rows_v.append(v)
    rp = np.zeros(A.numRows + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows_c])
    ci = np.concatenate(rows_c).astype(np.int32) if rows_c else np.zeros(0, np.int32)
    va = np.concatenate(rows_v) if rows_v else np.zeros(0)
    return adv.Csr(va, ci, rp, A.numRows, A.numCols)


def levels(A, lower=True):
    """level[i] = 1 + max level of the rows that row i's strict entries name (numpy's own sweep)."""
    m = A.numRows
    lev = np.zeros(m, np.int64)
    for r in (range(m) if lower else range(m - 1, -1, -1)):
        c = A.colIndices[A.rowPtr[r]:A.rowPtr[r + 1]]
        d = c[c < r] if lower else c[c > r]
        lev[r] = 1 + (lev[d].max() if d.size else 0)
    return lev


def order_of(lev):
    """Rows by level, ascending row index inside a level."""
    return np.argsort(lev, kind="stable")


def schedule(lev, thin, chain="auto"):
    """The launches of a schedule with threshold `thin`, restated: (launches,
    chain launches, rows in chain launches, most levels in one chain launch)."""
    w = np.bincount(lev)[1:] if lev.size else np.zeros(0, np.int64)
    is_thin = {"auto": w <= thin, "off": np.zeros(w.size, bool), "all": np.ones(w.size, bool)}[chain]
    launches = chains = rows = most = 0
    l = 0
    while l < w.size:
        e = l + 1
        if is_thin[l]:
            while e < w.size and is_thin[e]:
                e += 1
            chains += 1
            rows += int(w[l:e].sum())
            most = max(most, e - l)
        launches += 1
        l = e
    return launches, chains, rows, most


def counts(A, lower=True, unit=False):
    """(strict entries used, entries ignored, diagonal entries)."""
    r = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))
    c = A.colIndices
    strict = int(np.sum(c < r if lower else c > r))
    diag = 0 if unit else int(np.sum(c == r))
    return strict, int(c.size) - strict - diag, diag


def solve(A, X, lower=True, unit=False):
    """The reference: sequential substitution in CSR order, fp64, a separate
    multiply and subtract, the pivot summed over its duplicates in CSR order,
    one division."""
    m = A.numRows
    X = np.asarray(X, np.float64)
    Y = np.empty_like(X)
    rp, ci, va = A.rowPtr, A.colIndices, A.values
    with np.errstate(all="ignore"):
        for r in (range(m) if lower else range(m - 1, -1, -1)):
            s = X[r].copy()
            d = None
            for j in range(int(rp[r]), int(rp[r + 1])):
                c = ci[j]
                a = va[j]
                if (c < r) if lower else (c > r):
                    p = a * Y[c]
                    s = s - p
                elif c == r:
                    d = a if d is None else d + a
            Y[r] = s if unit else s / d
    return Y


# ---- inputs ---------------------------------------------------------------
@functools.lru_cache(None)
def band(long_rows=False):
    return freeze(with_diag(adv.adv_pattern(M, M, 1, adv.LONG_ROWS if long_rows else None), 7))


@functools.lru_cache(None)
def two_level():
    """Rows 0-63 a chain (row r names r - 1); every row >= 64 names row 63 and
    eight random rows < 64: 64 levels of one row, then one of 2,936."""
    rng = np.random.default_rng(5)
    rows = []
    for r in range(M):
        if r == 0:
            c = np.zeros(0, np.int64)
        elif r < 64:
            c = np.array([r - 1])
        else:
            c = np.concatenate([[63], rng.choice(64, 8, replace=True)])
            rng.shuffle(c)
        rows.append(np.asarray(c, np.int64))
    return freeze(with_diag(adv._csr(rows, rng, M, M), 8))


def _from_rows(rows, vals, m):
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    ci = (np.concatenate(rows) if rp[-1] else np.zeros(0)).astype(np.int32)
    return freeze(adv.Csr(np.asarray(vals, np.float64), ci, rp, m, m))


@functools.lru_cache(None)
def degenerate(case):
    """(A, unit_diag) of a degenerate shape."""
    rng = np.random.default_rng(11)
    if case == "m0":
        return _from_rows([], [], 0), False
    if case == "m1":
        return _from_rows([np.array([0])], [-1.75], 1), False
    if case == "nnz0_unit":  # Y = X
        return _from_rows([np.zeros(0, np.int64)] * 40, [], 40), True
    if case == "bidiagonal":  # 300 levels of one row (lower), entries unsorted in every other row
        rows, vals = [np.array([0])], [2.0]
        for r in range(1, 300):
            d, o = (2.0 + r % 3) * (-1.0 if r % 4 == 0 else 1.0), rng.uniform(-1, 1)
            rows.append(np.array([r, r - 1] if r % 2 else [r - 1, r]))
            vals += [d, o] if r % 2 else [o, d]
        return _from_rows(rows, vals, 300), False
    if case == "diagonal":  # one level
        return _from_rows([np.array([r]) for r in range(500)], rng.uniform(0.5, 2.0, 500) * np.where(np.arange(500) % 3, 1, -1), 500), False
    raise KeyError(case)


DEGENERATE = ("m0", "m1", "nnz0_unit", "bidiagonal", "diagonal")


@functools.lru_cache(None)
def x_full(m=M, seed=3):
    return _frozen(np.random.default_rng(seed).uniform(-1, 1, (m, KMAX)))


@functools.lru_cache(None)
def reference(name, lower=True, unit=False):
    """(A, X[m x 128], Y[m x 128]) of a named input; asserts the condition every
    bit-exact case rests on: the reference is at least 80 % finite."""
    if name == "band":
        A = band()
    elif name == "band_long":
        A = band(True)
    elif name == "two_level":
        A = two_level()
    else:
        A, unit = degenerate(name)
    X = x_full(A.numRows, 3)
    Y = _frozen(solve(A, X, lower, unit))
    assert Y.size == 0 or np.isfinite(Y).mean() >= 0.8
    return A, X, Y


@functools.lru_cache(None)
def reference2(lower=True):
    """`band` with other values on the same pattern (the changed values of the
    re-bind and replay cases): off-diagonal entries scaled by [0.5, 1), diagonal
    entries by [1, 1.5), so the diagonal stays dominant.  (A2, X, Y2)."""
    A = band()
    rng = np.random.default_rng(21)
    r = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))
    scale = np.where(A.colIndices == r, rng.uniform(1.0, 1.5, A.nnz), rng.uniform(0.5, 1.0, A.nnz))
    A2 = freeze(adv.Csr(A.values * scale, A.colIndices, A.rowPtr, A.numRows, A.numCols))
    X = x_full(M, 3)
    Y = _frozen(solve(A2, X, lower, False))
    assert np.isfinite(Y).all() and not np.array_equal(Y, reference("band", lower, False)[2])
    return A2, X, Y


@functools.lru_cache(None)
def special(lower=True):
    """Special values on `band`: values of +-0.0 and 2^+-600 (set before the
    diagonal is made dominant, so the solution stays bounded), one pivot that
    cancels to exactly +0.0 through its two duplicates, and X rows that are
    whole rows of +inf, -inf, NaN, -0.0, +0.0, 1e-310, 5e-324, +1.7e308 and -1.7e308.  The
    non-finite rows and the zero pivot lie in the last 5 % of the substitution
    order, so what they poison downstream stays under 20 % of Y."""
    A0 = adv.adv_pattern(M, M, 1)
    va = A0.values.copy()
    idx = np.arange(va.size)
    va[idx % 97 == 5] *= 2.0 ** 600
    va[idx % 97 == 50] *= 2.0 ** -600
    va[idx % 17 == 0] = 0.0
    va[idx % 17 == 1] = -0.0
    A = with_diag(adv.Csr(va, A0.colIndices, A0.rowPtr, M, M), 7)
    va = A.values.copy()
    tail = (lambda k: M - 150 + k) if lower else (lambda k: 149 - k)  # k-th row of the last 5 % of the order
    # the zero pivot: a row of the tail with two diagonal entries, a then -a
    zrow = next(r for r in (tail(k) for k in range(40, 150)) if r % 11 == 3)
    s, e = int(A.rowPtr[zrow]), int(A.rowPtr[zrow + 1])
    dpos = s + np.flatnonzero(A.colIndices[s:e] == zrow)
    assert dpos.size == 2
    va[dpos[0]], va[dpos[1]] = 1.5, -1.5
    X = np.array(x_full(M, 4))
    rows = {"+inf": (tail(60), np.inf), "-inf": (tail(75), -np.inf), "nan": (tail(90), np.nan),
            "+1.7e308": (tail(105), 1.7e308), "-1.7e308": (tail(120), -1.7e308),
            "-0": (1000, -0.0), "1e-310": (1250, 1e-310), "5e-324": (1500, 5e-324), "+0": (2001, 0.0)}
    for r, v in rows.values():
        X[r] = v
    # the four finite special rows keep what X gives them: every strict value
    # of theirs is +0.0 or -0.0 in turn, so s ends as a signed zero or the
    # tiny x, and the division gives a signed zero or a subnormal
    for r in (1000, 1250, 1500, 2001):
        s, e = int(A.rowPtr[r]), int(A.rowPtr[r + 1])
        off = s + np.flatnonzero(A.colIndices[s:e] != r)
        va[off] = np.where(np.arange(off.size) % 2, -0.0, 0.0)
    A = freeze(adv.Csr(va, A.colIndices, A.rowPtr, M, M))
    X = _frozen(X)
    Y = _frozen(solve(A, X, lower, False))
    fin = np.isfinite(Y)
    assert 0.8 <= fin.mean() < 1.0 and np.isnan(Y).any() and np.isinf(Y).any()
    info = {"zero_pivot_row": zrow, "x_rows": {k: r for k, (r, _) in rows.items()}}
    return A, X, Y, info
