"""Inputs and the independent reference for the reordering tests.

Plain numpy (no GPU, no torch, nothing from the library): the two rules of
include/smfv.h restated -- the first-fit greedy colouring of A + A^T in natural
order with a stable argsort by colour (multicolor), and the row-by-row
renumbering that keeps every row's CSR order (permute) -- on the matrices of
ilu0_ref, trsm_ref and adversarial plus a few small patterns of this file's
own.  Every input and reference is computed once, shared by the tests that
need it and handed out read-only.
"""
import functools
import os

import numpy as np

import adversarial as adv
import ilu0_ref as I
import trsm_ref as T

freeze = T.freeze
_frozen = T._frozen
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def multicolor(A):
    """(perm, color, ncolors): rows in natural order, color[i] the smallest
    c >= 0 no neighbour j < i in the graph of A + A^T (diagonal left out)
    holds; perm = rows by (color, row)."""
    m = A.numRows
    rp, ci = np.asarray(A.rowPtr), np.asarray(A.colIndices)
    rows = np.repeat(np.arange(m), np.diff(rp))
    # earlier[i]: the neighbours j < i of row i, from both (i, j) and (j, i)
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)
    keep = lo != hi
    order = np.argsort(hi[keep], kind="stable")
    lo, hi = lo[keep][order], hi[keep][order]
    start = np.searchsorted(hi, np.arange(m + 1))
    color = np.zeros(m, np.int64)
    for i in range(m):
        taken = set(color[lo[start[i]:start[i + 1]]].tolist())
        c = 0
        while c in taken:
            c += 1
        color[i] = c
    perm = np.argsort(color, kind="stable")
    return perm, color, (int(color.max()) + 1 if m else 0)


def permute(A, perm):
    """(B, vperm): row i of B is row perm[i] of A, entry by entry in A's CSR
    order, a column c renamed inv[c]."""
    m = A.numRows
    rp, ci = np.asarray(A.rowPtr), np.asarray(A.colIndices)
    perm = np.asarray(perm, np.int64)
    inv = np.empty(m, np.int64)
    inv[perm] = np.arange(m)
    b_rp, b_ci, vperm = [0], [], []
    for i in range(m):
        r = int(perm[i])
        for j in range(int(rp[r]), int(rp[r + 1])):
            b_ci.append(int(inv[ci[j]]))
            vperm.append(j)
        b_rp.append(len(b_ci))
    vperm = np.asarray(vperm, np.int64)
    B = adv.Csr(np.asarray(A.values)[vperm], np.asarray(b_ci, np.int32), np.asarray(b_rp, np.int32), m, m)
    return B, vperm


def dense(A):
    """The dense form of a small CSR (repeated entries summed)."""
    D = np.zeros((A.numRows, A.numCols))
    rows = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))
    np.add.at(D, (rows, A.colIndices), A.values)
    return D


# ---- inputs ---------------------------------------------------------------
def _from_rows(rows, m, seed=1):
    rng = np.random.default_rng(seed)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    ci = (np.concatenate([np.asarray(c, np.int64) for c in rows]) if rp[-1] else np.zeros(0)).astype(np.int32)
    return freeze(adv.Csr(rng.uniform(-1, 1, ci.size), ci, rp, m, m))


@functools.lru_cache(None)
def sym5():
    """tests/golden/sym5.mtx (coordinate, symmetric: the lower triangle is stored), read here."""
    ent = []
    with open(os.path.join(GOLDEN, "sym5.mtx")) as f:
        header = f.readline().lower()
        lines = [ln for ln in f if not ln.startswith("%")]
    m, n, _ = (int(t) for t in lines[0].split())
    for ln in lines[1:]:
        t = ln.split()
        if not t:
            continue
        r, c, v = int(t[0]) - 1, int(t[1]) - 1, float(t[2]) if len(t) > 2 else 1.0
        ent.append((r, c, v))
        if "symmetric" in header and r != c:
            ent.append((c, r, v))
    ent.sort()
    rows = [[c for r, c, _ in ent if r == i] for i in range(m)]
    A = _from_rows(rows, m)
    return freeze(adv.Csr(np.array([v for _, _, v in ent]), A.colIndices, A.rowPtr, m, n))


@functools.lru_cache(None)
def one_sided():
    """Not structurally symmetric: a chain stored in one direction only, half
    of it as (i, i - 1) and half as (i - 1, i), plus (0, m - 1) with no
    (m - 1, 0).  Every stored pair must separate its two rows."""
    m = 41  # odd: row m - 1 sees both colours of the chain
    rows = [[] for _ in range(m)]
    for i in range(1, m):
        if i % 2:
            rows[i].append(i - 1)
        else:
            rows[i - 1].append(i)
    rows[0].append(m - 1)
    return _from_rows(rows, m, 2)


@functools.lru_cache(None)
def repeated_unsorted():
    """Rows with repeated and unsorted columns, the diagonal repeated too."""
    rows = [[3, 0, 3, 1], [1, 1, 0], [5, 2, 4, 5, 2], [0], [2, 4, 4], [5, 0, 2], [6, 6, 6], [1, 7, 6, 1]]
    return _from_rows(rows, 8, 3)


@functools.lru_cache(None)
def empty_rows():
    """Empty rows between coupled ones, first and last row empty."""
    rows = [[], [2, 1], [], [1, 5], [], [3, 6], [5], [], []]
    return _from_rows(rows, 9, 4)


@functools.lru_cache(None)
def adversarial_square():
    """The square adversarial pattern (unsorted rows, non-adjacent repeated
    columns, empty rows, two long rows)."""
    return freeze(adv.adv_pattern(T.M, T.M, 1, adv.LONG_ROWS))


SMALL = {"sym5": sym5, "one_sided": one_sided, "repeated_unsorted": repeated_unsorted, "empty_rows": empty_rows,
         "m0": lambda: I.degenerate("m0"), "m1": lambda: I.degenerate("m1")}
INPUTS = {"band": I.band, "grid9": I.grid9, "long_row": I.long_row, "wide": I.wide, "trsm_band": T.band,
          "adversarial": adversarial_square, **SMALL}


@functools.lru_cache(None)
def ordering(name):
    """(perm, color, ncolors) of a named input, by this file's rule."""
    perm, color, nc = multicolor(INPUTS[name]())
    return _frozen(perm), _frozen(color), nc


@functools.lru_cache(None)
def renumbered(name):
    """(B, vperm) of a named input under its multicolour ordering."""
    B, vperm = permute(INPUTS[name](), ordering(name)[0])
    return freeze(B), _frozen(vperm)
