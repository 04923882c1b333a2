"""Inputs and the independent reference for the ILU(0) tests.

Plain numpy (no GPU, no torch, nothing from the library): the loop of
include/smfv.h over CSR entries (factor), recounts of steps, pairs and levels
(counts), and the test matrices.  Every input and reference is computed once,
shared by the tests that need it and handed out read-only.
"""
import functools

import numpy as np

import adversarial as adv
import trsm_ref as T

M = 3000
SLOT = 256  # entries of a wavefront's LDS slot (include/smfv.h): longer rows are long rows

freeze = T.freeze
_frozen = T._frozen


def factor(A):
    """The reference: for every row, its strict-lower entries in ascending
    column; a true division, then a separate multiply and subtract on every
    entry of row k right of k whose column row i holds.  Returns f in CSR
    order."""
    m, rp, ci = A.numRows, A.rowPtr, A.colIndices
    a = np.asarray(A.values, np.float64)
    f = np.empty_like(a)
    diag = np.full(m, -1, np.int64)
    with np.errstate(all="ignore"):
        for i in range(m):
            s, e = int(rp[i]), int(rp[i + 1])
            cols = ci[s:e].tolist()
            w = a[s:e].copy()
            pos = {c: t for t, c in enumerate(cols)}
            assert len(pos) == len(cols) and i in pos, i
            diag[i] = s + pos[i]
            for k, t in sorted((c, t) for t, c in enumerate(cols) if c < i):
                w[t] = w[t] / f[diag[k]]
                for q in range(int(rp[k]), int(rp[k + 1])):
                    c = int(ci[q])
                    r = pos.get(c) if c > k else None
                    if r is not None:
                        prod = w[t] * f[q]
                        w[r] = w[r] - prod
            f[s:e] = w
    return f


def counts(A):
    return _count(A)


@functools.lru_cache(None)
def levels(name):
    """trsm_ref.levels (lower) of a named input, computed once."""
    return _frozen(T.levels(special()[0] if name == "special" else INPUTS[name]()))


@functools.lru_cache(None)
def counts_of(name):
    """counts() of a named input, computed once."""
    return _count(special()[0] if name == "special" else INPUTS[name]())


def _count(A):
    """{steps, pairs, max_steps, max_pairs, long_rows}, recounted with sorted
    columns and set intersections (not the reference's dictionary)."""
    m, rp, ci = A.numRows, A.rowPtr, A.colIndices
    upper = [np.sort(ci[rp[k]:rp[k + 1]][ci[rp[k]:rp[k + 1]] > k]) for k in range(m)]
    steps = pairs = max_steps = max_pairs = long_rows = 0
    for i in range(m):
        c = ci[rp[i]:rp[i + 1]]
        low = c[c < i]
        mine = np.sort(c)
        n = sum(int(np.isin(upper[k], mine, assume_unique=True).sum()) for k in low)
        steps += low.size
        pairs += n
        max_steps, max_pairs = max(max_steps, int(low.size)), max(max_pairs, n)
        long_rows += int(c.size > SLOT)
    return {"steps": int(steps), "pairs": int(pairs), "max_steps": max_steps, "max_pairs": max_pairs,
            "long_rows": long_rows}


def split(A, f):
    """(L, U) as DeviceCSR-independent host matrices of A's pattern: the values
    the two solves see are f itself (lower unit-diagonal ignores the diagonal)."""
    return adv.Csr(f, A.colIndices, A.rowPtr, A.numRows, A.numCols)


# ---- inputs ---------------------------------------------------------------
def _finish(rows_c, rows_v, m, seed, shuffle=True):
    """Per row: the diagonal entry added where missing, the entry order
    shuffled, diagonal = +-(1 + sum |off-diagonal|)."""
    rng = np.random.default_rng(seed)
    out_c, out_v = [], []
    for r in range(m):
        c, v = np.asarray(rows_c[r], np.int64), np.asarray(rows_v[r], np.float64)
        if not (c == r).any():
            c, v = np.append(c, r), np.append(v, 0.0)
        if shuffle:
            o = rng.permutation(c.size)
            c, v = c[o], v[o]
        v = v.copy()
        off = c != r
        v[~off] = (-1.0 if r % 5 == 0 else 1.0) * (1.0 + np.abs(v[off]).sum())
        out_c.append(c)
        out_v.append(v)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in out_c])
    ci = (np.concatenate(out_c) if m else np.zeros(0)).astype(np.int32)
    va = np.concatenate(out_v) if m else np.zeros(0)
    return adv.Csr(va, ci, rp, m, m)


def _dedup(A):
    """Each row's repeated columns removed (the first occurrence stays)."""
    rows_c, rows_v = [], []
    for r in range(A.numRows):
        s, e = int(A.rowPtr[r]), int(A.rowPtr[r + 1])
        _, first = np.unique(A.colIndices[s:e], return_index=True)
        first = np.sort(first)
        rows_c.append(A.colIndices[s:e][first])
        rows_v.append(A.values[s:e][first])
    return rows_c, rows_v


@functools.lru_cache(None)
def band():
    rows_c, rows_v = _dedup(adv.adv_pattern(M, M, 1))
    return freeze(_finish(rows_c, rows_v, M, 7))


@functools.lru_cache(None)
def band2():
    """Other values on `band`'s pattern: off-diagonal entries scaled by
    [0.5, 1), diagonal entries by [1, 1.5) (the diagonal stays dominant)."""
    A = band()
    rng = np.random.default_rng(21)
    r = np.repeat(np.arange(M), np.diff(A.rowPtr))
    scale = np.where(A.colIndices == r, rng.uniform(1.0, 1.5, A.nnz), rng.uniform(0.5, 1.0, A.nnz))
    return freeze(adv.Csr(A.values * scale, A.colIndices, A.rowPtr, M, M))


@functools.lru_cache(None)
def grid9(n=24):
    """The 9-point stencil on an n x n grid, rows shuffled inside."""
    rng = np.random.default_rng(9)
    rows_c, rows_v = [], []
    for y in range(n):
        for x in range(n):
            c = [yy * n + xx for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1) if 0 <= yy < n and 0 <= xx < n]
            rows_c.append(np.array(c))
            rows_v.append(rng.uniform(-1, 1, len(c)))
    return freeze(_finish(rows_c, rows_v, n * n, 10))


@functools.lru_cache(None)
def long_row():
    """An arrow: tridiagonal, with the last row and the last column full."""
    rng = np.random.default_rng(12)
    rows_c = [np.unique([c for c in (r - 1, r, r + 1, M - 1) if 0 <= c < M]) for r in range(M - 1)] + [np.arange(M)]
    rows_v = [rng.uniform(-1, 1, len(c)) for c in rows_c]
    return freeze(_finish(rows_c, rows_v, M, 13))


@functools.lru_cache(None)
def wide():
    """Block-diagonal, 8 x 8 dense blocks."""
    rng = np.random.default_rng(14)
    rows_c = [np.arange(r // 8 * 8, r // 8 * 8 + 8) for r in range(M)]
    rows_v = [rng.uniform(-1, 1, 8) for _ in range(M)]
    return freeze(_finish(rows_c, rows_v, M, 15))


@functools.lru_cache(None)
def degenerate(case):
    rng = np.random.default_rng(16)
    if case == "m0":
        return freeze(adv.Csr(np.zeros(0), np.zeros(0, np.int32), np.zeros(1, np.int32), 0, 0))
    if case == "m1":
        return freeze(adv.Csr(np.array([-1.75]), np.zeros(1, np.int32), np.array([0, 1], np.int32), 1, 1))
    if case == "diagonal":  # one level, no steps
        m = 500
        return freeze(_finish([np.array([r]) for r in range(m)], [rng.uniform(-1, 1, 1) for _ in range(m)], m, 17))
    if case == "upper_bidiagonal":  # no steps: every row is copied
        m = 300
        rows_c = [np.array([r + 1, r] if r % 2 else [r, r + 1]) if r + 1 < m else np.array([r]) for r in range(m)]
        A = _finish(rows_c, [rng.uniform(-1, 1, len(c)) for c in rows_c], m, 18, shuffle=False)
        return freeze(A)
    raise KeyError(case)


DEGENERATE = ("m0", "m1", "diagonal", "upper_bidiagonal")


@functools.lru_cache(None)
def special():
    """`band`'s pattern with special values, all in the last 5 % of the rows:
    values of +-0.0, 2^+-600 and subnormals, one pivot exactly +0.0, one NaN
    and one +inf entry."""
    A = band()
    va = np.array(A.values)
    rp, ci = A.rowPtr, A.colIndices
    lo = int(rp[M - 150])
    idx = np.arange(va.size)
    r = np.repeat(np.arange(M), np.diff(rp))
    offd = (ci != r) & (idx >= lo)
    va[offd & (idx % 13 == 0)] = 0.0
    va[offd & (idx % 13 == 1)] = -0.0
    va[offd & (idx % 13 == 2)] *= 2.0 ** 600
    va[offd & (idx % 13 == 3)] *= 2.0 ** -600
    va[offd & (idx % 13 == 4)] *= 2.0 ** -1040  # subnormal
    zrow = M - 20
    va[int(rp[zrow]) + int(np.flatnonzero(ci[rp[zrow]:rp[zrow + 1]] == zrow)[0])] = 0.0
    cand = np.flatnonzero(offd & (r >= M - 60) & (idx % 13 > 4))
    va[cand[0]] = np.nan
    va[cand[len(cand) // 2]] = np.inf
    return freeze(adv.Csr(va, ci, rp, M, M)), {"zero_pivot_row": zrow}


INPUTS = {"band": band, "grid9": grid9, "long_row": long_row, "wide": wide, "band2": band2,
          **{c: (lambda c=c: degenerate(c)) for c in DEGENERATE}}


@functools.lru_cache(None)
def reference(name):
    """(A, f) of a named input."""
    if name == "special":
        A, _ = special()
        f = _frozen(factor(A))
        assert np.isfinite(f).mean() >= 0.8 and np.isnan(f).any() and np.isinf(f).any()
        return A, f
    A = INPUTS[name]()
    f = _frozen(factor(A))
    assert np.isfinite(f).all()
    return A, f


@functools.lru_cache(None)
def applied(name, K=40):
    """(X, Y): U^-1 L^-1 X by trsm_ref.solve applied twice to the reference factors."""
    A, f = reference(name)
    Fm = split(A, f)
    X = _frozen(np.random.default_rng(31).uniform(-1, 1, (A.numRows, K)))
    Y = _frozen(T.solve(Fm, T.solve(Fm, X, True, True), False, False))
    assert np.isfinite(Y).all()
    return X, Y
