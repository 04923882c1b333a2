"""Adversarial inputs and independent references for the parity tests.

Plain numpy (no GPU, no torch, nothing from oracle/): patterns with
unsorted rows and non-adjacent repeated columns, values and X rows holding
signed zeros, subnormals, 2^+-600, +-inf, NaN and +-1.7e308, rows built so
that the reference sum is exactly +0.0, and two references that restate
SC/SparseMatrixFatVectorMultiply.cpp:17-27 as a loop over each row's entries
in CSR order: ref_f64 (the bit-exact reference) and ref_hi (np.longdouble,
for the tolerance paths).
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class Csr:
    values: np.ndarray
    colIndices: np.ndarray
    rowPtr: np.ndarray
    numRows: int
    numCols: int

    @property
    def nnz(self):
        return int(self.rowPtr[-1])


LONG_ROWS = {100: 700, 2000: 1300}  # rows too wide for a tile: the direct list
WIDE_ROW = 82  # the row [n-1, 0, n-1]


# Leading dimensions (doubles, all even) of test_gpu_large_offsets.py: a
# column window of a 3,000-row buffer with one of these strides spans n*ld*8
# bytes, on a chosen side of the kernels' 2 GiB / 4 GiB addressing switches.
LARGE_N = 3000
LARGE_LD = {"A": 89478,    # just under 2^31: k_rows_mh's buffer form at its highest offsets
            "B": 89480,    # just over 2^31: its 64-bit pointer form; k_rows_ws scalar-base form
            "C": 178956,   # just under 2^32: scalar-base / wsn / live at their highest offsets
            "D": 178958,   # just over 2^32: the dispatch flips; no offset reaches 2^32 yet
            "E": 268436}   # 6 GiB: columns >= 2,000 lie beyond 2^32


def large_offset_conditions(A):
    """The conditions the large-offset cases rest on, for the pattern A (n =
    LARGE_N): every span on its side of its threshold, and at least a quarter
    of A's entries read X at a byte offset >= 2^31 with ld C, >= 2^32 with ld
    E.  Returns the two shares."""
    ld, n = LARGE_LD, LARGE_N
    assert A.numCols == n and all(v % 2 == 0 for v in ld.values())
    span = {k: n * v * 8 for k, v in ld.items()}
    assert span["A"] <= 0x7fffffff < span["B"] < 1 << 32
    assert 1 << 31 < span["C"] < 1 << 32 <= span["D"] < span["E"]
    assert (1 << 32) - span["C"] < 2 * 8 * n and span["D"] - (1 << 32) < 2 * 8 * n  # two doubles a row from 2^32
    assert 0x7fffffff - span["A"] < 2 * 8 * n and span["B"] - (1 << 31) < 2 * 8 * n
    assert (n - 1) * ld["D"] * 8 < 1 << 32 < (n - 1) * ld["E"] * 8
    off = A.colIndices.astype(np.int64) * 8
    share_c = float(np.mean(off * ld["C"] >= 1 << 31))
    share_e = float(np.mean(off * ld["E"] >= 1 << 32))
    assert share_c >= 0.25 and share_e >= 0.25, (share_c, share_e)
    assert (n - 1) * (ld["E"] - 1) * 8 >= 1 << 32  # the odd ld E - 1
    return share_c, share_e


def _csr(rows, vals_rng, m, n):
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    ci = (np.concatenate(rows) if rp[-1] else np.zeros(0)).astype(np.int32)
    return Csr(vals_rng.uniform(-1, 1, ci.size), ci, rp, m, n)


def adv_pattern(m, n, seed, long_rows=None):
    """Row lengths arange(m) % 41 (every residue mod 8, empty rows), columns
    from a +-40 band around r*n//m; every 7th row appends its first and last
    column again (non-adjacent repeats) and every row is shuffled (unsorted);
    row WIDE_ROW is [n-1, 0, n-1]; long_rows maps a row to its length, columns
    drawn over all of n.  Values uniform in [-1, 1)."""
    rng = np.random.default_rng(seed)
    long_rows = long_rows or {}
    rows = []
    for r in range(m):
        L = r % 41
        if r in long_rows:
            cols = rng.choice(n, long_rows[r], replace=long_rows[r] > n)
        elif r == WIDE_ROW:
            cols = np.array([n - 1, 0, n - 1])
        else:
            c = r * n // m
            band = np.arange(max(0, c - 40), min(n, c + 41))
            cols = rng.choice(band, L, replace=L > band.size)
            if r % 7 == 0 and L:
                cols = np.concatenate([cols, cols[:1], cols[-1:]])
            rng.shuffle(cols)
        rows.append(np.asarray(cols, np.int64))
    return _csr(rows, rng, m, n)


def adv_degenerate(m, n, seed):
    """1 x 500 (one 300-entry row), 500 x 1, 1 x 1, 2000 x 3: random columns,
    hence repeats; every 5th value -0.0, every 7th +0.0."""
    rng = np.random.default_rng(seed)
    lens = np.full(m, 300) if m == 1 and n > 1 else np.arange(m) % 5 if m > 1 else np.ones(1, int)
    A = _csr([rng.integers(0, n, int(L)) for L in lens], rng, m, n)
    idx = np.arange(A.nnz)
    A.values[idx % 5 == 0] = -0.0
    A.values[idx % 7 == 0] = 0.0
    return A


def adv_values(A, X, finite_only=False):
    """Special values for the pattern A (m, n >= 1000) and the dense X:
    returns (A', X', info).

    A: every 17th value +0.0, the next residue class -0.0, 2^600 and 2^-600
    scaled values scattered through the rest.  X: one whole row each of +inf,
    -inf, NaN, -0.0, +0.0, 5e-324, 1e-310, +1.7e308, -1.7e308; ten rows scaled
    by 2^-1060 (subnormal).  Beyond that, `poison_rows`: six rows that follow a
    row of odd length start with a value of NaN or -inf.  finite_only drops
    the inf / NaN / +-1.7e308 rows of X and the poison in A.

    Constructed rows (info): `negzero_rows`, every product -0.0 (half of them
    a value of -0.0 times a positive x, half a positive value times an x of
    -0.0); `cancel_rows`, a*x followed by (-a)*x over equal X rows with a a
    power of two, so the products are exact and the row is +0.0 with and
    without a fused multiply-add; `subnormal_rows`, one entry 2^-1040 times a
    normal x.  A constructed row never shares an X row with a special row or
    with another constructed row."""
    m, n = A.numRows, A.numCols
    assert m >= 1000 and n >= 1000
    rp, ci = A.rowPtr, A.colIndices
    va, X = A.values.copy(), np.array(X, dtype=np.float64)
    K = X.shape[1]
    idx = np.arange(va.size)
    va[idx % 97 == 5] *= 2.0 ** 600
    va[idx % 97 == 50] *= 2.0 ** -600
    va[idx % 17 == 0] = 0.0
    va[idx % 17 == 1] = -0.0
    pos = lambda k: k * n // 40  # noqa: E731
    special = {"+inf": (pos(3), np.inf), "-inf": (pos(7), -np.inf), "nan": (pos(11), np.nan),
               "-0": (pos(15), -0.0), "+0": (pos(19), 0.0), "5e-324": (pos(23), 5e-324),
               "1e-310": (pos(27), 1e-310), "+1.7e308": (pos(31), 1.7e308), "-1.7e308": (pos(35), -1.7e308)}
    tiny = [pos(4 * k + 2) for k in range(10)]
    taken = {p for p, _ in special.values()} | set(tiny)
    # constructed rows: greedy, each claims its X rows
    want = {"neg_a": 12, "neg_x": 12, "cancel": 24, "sub": 8}
    got = {k: [] for k in want}
    xc = np.random.default_rng(n).uniform(0.5, 1.0, K)
    next_r = 0  # spread the constructed rows over the matrix (many tiles, every row block)
    for r in range(m):
        s, e = int(rp[r]), int(rp[r + 1])
        L = e - s
        if L == 0 or L > 12 or r == WIDE_ROW or r < next_r:
            continue
        cols = set(ci[s:e].tolist())
        if cols & taken:
            continue
        kinds = [k for k in (("sub",) if L == 1 else ("neg_a", "neg_x", "cancel")) if len(got[k]) < want[k]]
        if L % 2:
            kinds = [k for k in kinds if k != "cancel"]
        if L > 5:
            kinds = [k for k in kinds if k != "neg_x"]
        if not kinds:
            continue
        kind = min(kinds, key=lambda k: len(got[k]) / want[k])
        got[kind].append(r)
        next_r = r + m // 100
        taken |= cols
        c = sorted(cols)
        if kind == "neg_a":    # -0.0 * positive x
            va[s:e] = -0.0
            X[c] = np.where(X[c] == 0.0, 0.5, np.abs(X[c]))
        elif kind == "neg_x":  # positive a * -0.0
            va[s:e] = np.where(va[s:e] == 0.0, 0.5, np.abs(va[s:e]))
            X[c] = -0.0
        elif kind == "cancel":  # a*x then (-a)*x, a a power of two
            a = 2.0 ** ((np.arange(L // 2) % 7) - 3.0)
            va[s:e:2], va[s + 1:e:2] = a, -a
            X[c] = xc
        else:                  # one subnormal product
            va[s] = 2.0 ** -1040
    assert all(len(got[k]) == want[k] for k in want), {k: len(v) for k, v in got.items()}
    # NaN / -inf as the first value of rows that follow rows of odd length: a
    # live-values plan reads it as the second half of the odd row's last pair
    built = {r for rows_ in got.values() for r in rows_}
    poison = []
    for r0 in range(m // 7, m - m // 7 + 1, m // 7):
        r = next(r for r in range(r0, m) if (rp[r] - rp[r - 1]) % 2 == 1 and rp[r + 1] > rp[r]
                 and not {r - 1, r} & built)
        poison.append(r)
        if not finite_only:
            va[rp[r]] = np.nan if len(poison) % 2 else -np.inf
    for name, (p, v) in special.items():
        if finite_only and not (np.isfinite(v) and abs(v) < 1e300):
            continue
        X[p] = v
    X[tiny] *= 2.0 ** -1060
    info = {"negzero_rows": np.array(got["neg_a"] + got["neg_x"]), "cancel_rows": np.array(got["cancel"]),
            "subnormal_rows": np.array(got["sub"]), "poison_rows": np.array(poison),
            "x_special": {k: p for k, (p, _) in special.items()}}
    info["zero_rows"] = np.concatenate([info["negzero_rows"], info["cancel_rows"]])
    return Csr(va, ci, rp, m, n), X, info


def _ref(A, X, dtype):
    va, Xd = A.values.astype(dtype), np.asarray(X).astype(dtype)
    rp, ci = A.rowPtr, A.colIndices
    Y = np.zeros((A.numRows, Xd.shape[1]), dtype)
    with np.errstate(all="ignore"):
        for r in range(A.numRows):
            s = np.zeros(Xd.shape[1], dtype)
            for j in range(int(rp[r]), int(rp[r + 1])):
                s = s + va[j] * Xd[ci[j]]
            Y[r] = s
    return Y


def ref_f64(A, X):
    """s = 0.0; s = s + a * X[c] over the row's entries in CSR order, fp64."""
    return _ref(A, X, np.float64)


def ref_hi(A, X):
    """The same loop in np.longdouble (rows of finite scale only)."""
    return _ref(A, X, np.longdouble)


def scale_hi(A, X):
    """sum |a||x| per row and column (np.longdouble), the tolerance's scale."""
    with np.errstate(all="ignore"):
        return _ref(Csr(np.abs(A.values), A.colIndices, A.rowPtr, A.numRows, A.numCols), np.abs(X), np.longdouble)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(Y, Yref):
    """NaN exactly where the reference has NaN; identical bits everywhere
    else, the sign of zero and +-inf included."""
    Y, Yref = np.asarray(Y), np.asarray(Yref)
    nan = np.isnan(Yref)
    return Y.shape == Yref.shape and np.array_equal(np.isnan(Y), nan) and np.array_equal(bits(Y)[~nan], bits(Yref)[~nan])


def within_tol(Y, Yhi, scale, Yref, tol=1e-12, floor=1e-300):
    """The tolerance paths' check (tests/test_gpu_parity.py's own tolerance
    and floor): |Y - Yhi| <= 1e-12 x sum|a||x| + 1e-300 on the elements whose
    scale is finite and below 1e300; on the others Y is non-finite wherever
    the fp64 reference Yref is.  Returns (ok, worst error / bound)."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(scale) & (scale < 1e300)
        err = np.abs(np.asarray(Y).astype(np.longdouble) - Yhi)
        bound = tol * scale + np.longdouble(floor)
        ok = bool(np.all(err[fin] <= bound[fin]))
        worst = float(np.max(err[fin] / bound[fin])) if fin.any() else 0.0
    rest = ~fin & ~np.isfinite(Yref)
    return ok and bool(np.all(~np.isfinite(np.asarray(Y)[rest]))), worst
