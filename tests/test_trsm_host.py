"""Host-side checks of the triangular solves (smfv_trsm_*): the library's
levels and order against numpy's own sweep on every test input and both
triangles, the analysis figures (schedule, entry counts) against the same
computation, the refusals, symbols and constants, the Python surface that
needs no device, the code-object notes of the new kernels and a sanitizer
build of the host analysis as a stand-alone program.  No GPU.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trsm_ref as T  # noqa: E402
from test_transpose_host import _kernel_notes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsematrixmultiplicationmpi_amd")
CSRC = os.path.join(PKG, "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
SMFV_ERR_INVALID = -1
IP = ctypes.POINTER(ctypes.c_int)
PD = ctypes.POINTER(ctypes.c_double)
UPPER, UNIT, NO_CHAIN, CHAIN_ALL, NSTATS = 1, 2, 4, 8, 12

INPUTS = {"band": lambda: T.band(), "band_long": lambda: T.band(True), "two_level": T.two_level,
          **{c: (lambda c=c: T.degenerate(c)[0]) for c in T.DEGENERATE}}


def _lib():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    lib.smfv_trsm_levels.restype = ctypes.c_int
    lib.smfv_trsm_levels.argtypes = [ctypes.c_int, IP, IP, ctypes.c_int, IP, IP, IP]
    lib.smfv_trsm_analyse.restype = ctypes.c_int
    lib.smfv_trsm_analyse.argtypes = [ctypes.c_int, IP, IP, ctypes.c_int, ctypes.c_int, PD]
    lib.smfv_last_error.restype = ctypes.c_char_p
    return lib


def _levels(lib, A, flags, ci=None):
    m = A.numRows
    rp = np.ascontiguousarray(A.rowPtr, np.int32)
    ci = np.ascontiguousarray(A.colIndices if ci is None else ci, np.int32)
    level, order = np.full(m, -7, np.int32), np.full(m, -7, np.int32)
    n = ctypes.c_int(-7)
    rc = lib.smfv_trsm_levels(m, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), flags, level.ctypes.data_as(IP),
                              order.ctypes.data_as(IP), ctypes.byref(n))
    return rc, level, order, n.value


def _analyse(lib, A, K, flags, ci=None):
    rp = np.ascontiguousarray(A.rowPtr, np.int32)
    ci = np.ascontiguousarray(A.colIndices if ci is None else ci, np.int32)
    out = np.full(NSTATS, -7.0)
    rc = lib.smfv_trsm_analyse(A.numRows, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), K, flags, out.ctypes.data_as(PD))
    return rc, out


def test_input_facts():
    """What the inputs are for (checked against the figures the cases were designed with)."""
    A = T.band()
    lens = np.diff(A.rowPtr)
    r = np.repeat(np.arange(A.numRows), lens)
    ndiag = np.bincount(r[A.colIndices == r], minlength=A.numRows)
    assert ndiag.min() == 1 and (ndiag == 2).sum() >= 3000 // 11 and (A.colIndices < r).any() and (A.colIndices > r).any()
    unsorted = sum(bool(np.any(np.diff(A.colIndices[A.rowPtr[i]:A.rowPtr[i + 1]]) < 0)) for i in range(A.numRows))
    assert unsorted > 1000
    for lower, nlev in ((True, 953), (False, 946)):
        lev = T.levels(A, lower)
        w = np.bincount(lev)[1:]
        assert lev.max() == nlev and 148 <= w.max() <= 152 and int(np.median(w)) == 3
        _, _, Y = T.reference("band", lower, False)
        assert np.isfinite(Y).all() and 1.0 < np.abs(Y).max() < 2.0
        _, _, Yu = T.reference("band", lower, True)
        assert np.isfinite(Yu).all() and 1e40 < np.abs(Yu).max() < 1e50
    assert np.diff(T.band(True).rowPtr).max() >= 1300
    lev = T.levels(T.two_level())
    w = np.bincount(lev)[1:]
    assert lev.max() == 65 and (w[:64] == 1).all() and w[64] == 2936
    assert T.levels(T.degenerate("bidiagonal")[0]).max() == 300 and T.levels(T.degenerate("diagonal")[0]).max() == 1
    for lower in (True, False):  # the special-values case keeps its poison in the tail
        _, _, Y, info = T.special(lower)
        assert 0.8 <= np.isfinite(Y).mean() < 1.0
        z = info["zero_pivot_row"]
        assert not np.isfinite(Y[z]).any()


@pytest.mark.parametrize("uplo", ["lower", "upper"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_levels_match_numpy(name, uplo):
    A = INPUTS[name]()
    lev = T.levels(A, uplo == "lower")
    rc, level, order, n = _levels(_lib(), A, UPPER if uplo == "upper" else 0)
    assert rc == 0
    assert n == (int(lev.max()) if lev.size else 0)
    assert np.array_equal(level, lev)
    assert np.array_equal(order, T.order_of(lev))


@pytest.mark.parametrize("chain", ["auto", "off", "all"])
@pytest.mark.parametrize("name,uplo,unit", [(n, u, d) for n in INPUTS for u in ("lower", "upper") for d in (False, True)
                                            if d or n != "nnz0_unit"])  # (no diagonal: refused without UNIT_DIAG)
def test_analyse_matches_numpy(name, uplo, unit, chain):
    A = INPUTS[name]()
    lower = uplo == "lower"
    flags = (0 if lower else UPPER) | (UNIT if unit else 0) | {"auto": 0, "off": NO_CHAIN, "all": CHAIN_ALL}[chain]
    rc, out = _analyse(_lib(), A, 32, flags)
    assert rc == 0, _lib().smfv_last_error()
    lev = T.levels(A, lower)
    w = np.bincount(lev)[1:] if lev.size else np.zeros(1, np.int64)
    thin = int(out[11])
    assert thin >= 1
    launches, chains, rows, most = T.schedule(lev, thin, chain)
    strict, ignored, diag = T.counts(A, lower, unit)
    assert [int(v) for v in out[:9]] == [int(lev.max()) if lev.size else 0, int(w.max()), launches, chains, rows, most,
                                         strict, ignored, diag]
    assert out[9] == 0 and out[10] >= 0
    if chain == "off":
        assert launches == (int(lev.max()) if lev.size else 0) and chains == 0
    if chain == "all" and lev.size:
        assert launches == 1 and rows == A.numRows


def test_thin_rows_setting():
    """SMFV_TRSM_THIN_ROWS moves levels between the two kernels and nothing else."""
    A = T.band()
    lev = T.levels(A)
    seen = set()
    for thin in (1, 3, 64, 200):
        rc, out = _analyse(_lib(), A, 32, thin << 8)
        assert rc == 0 and int(out[11]) == thin
        assert tuple(int(v) for v in out[2:6]) == T.schedule(lev, thin)
        seen.add(int(out[2]))
    assert len(seen) >= 3
    assert _analyse(_lib(), A, 32, 200 << 8)[1][2] == 1  # every level of `band` is thinner than 200 rows


def test_refusals():
    lib = _lib()
    A = T.band()
    # a structurally missing diagonal: the first such row is named
    ci = A.colIndices.copy()
    r = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))
    for row in (1711, 412):
        ci[(r == row) & (ci == row)] = row - 1
    for flags in (0, UPPER, NO_CHAIN, CHAIN_ALL):
        rc, out = _analyse(lib, A, 8, flags, ci)
        assert rc == SMFV_ERR_INVALID and (out == -7).all()
        msg = lib.smfv_last_error().decode()
        assert "row 412 " in msg and "diagonal" in msg, msg
    assert _analyse(lib, A, 8, UNIT, ci)[0] == 0
    # a column outside [0, m)
    for bad in (A.numRows, -1):
        ci = A.colIndices.copy()
        ci[ci.size // 2] = bad
        rc, _ = _analyse(lib, A, 8, 0, ci)
        assert rc == SMFV_ERR_INVALID and f"column index {bad} " in lib.smfv_last_error().decode()
        rc, level, order, _ = _levels(lib, A, 0, ci)
        assert rc == SMFV_ERR_INVALID and (level == -7).all() and (order == -7).all()
    for K in (0, -1):
        assert _analyse(lib, A, K, 0)[0] == SMFV_ERR_INVALID and "K" in lib.smfv_last_error().decode()
    assert _analyse(lib, A, 8, NO_CHAIN | CHAIN_ALL)[0] == SMFV_ERR_INVALID
    assert _analyse(lib, A, 8, 1 << 28)[0] == SMFV_ERR_INVALID


def test_create_refuses_before_any_device_call():
    """smfv_trsm_plan_create answers SMFV_ERR_INVALID -- not a HIP error, which
    is what a device call would give where there is no device -- and makes no
    plan: the pattern, the diagonal and K are checked on the host first."""
    lib = _lib()
    lib.smfv_trsm_plan_create.restype = ctypes.c_int
    lib.smfv_trsm_plan_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int64, IP, IP,
                                          ctypes.c_int, ctypes.c_int]
    A = T.band()
    rp = np.ascontiguousarray(A.rowPtr, np.int32)
    r = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))
    no_diag, bad_col = A.colIndices.copy(), A.colIndices.copy()
    no_diag[(r == 99) & (no_diag == 99)] = 98
    bad_col[7] = A.numRows
    for ci, K, word in ((no_diag, 32, "row 99 "), (bad_col, 32, "column index 3000 "), (A.colIndices, 0, "K = 0")):
        h = ctypes.c_void_p()
        ci = np.ascontiguousarray(ci, np.int32)
        rc = lib.smfv_trsm_plan_create(ctypes.byref(h), A.numRows, A.nnz, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), K, 0)
        assert rc == SMFV_ERR_INVALID and not h.value and word in lib.smfv_last_error().decode()


def test_trsm_symbols_and_constants():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    names = ("smfv_trsm_plan_create", "smfv_trsm_plan_bind_values", "smfv_trsm_plan_execute", "smfv_trsm_plan_stats",
             "smfv_trsm_plan_destroy", "smfv_trsm_analyse", "smfv_trsm_levels")
    for name in names:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "smfv.h")) as f:
        src = f.read()
    for macro, value in (("SMFV_TRSM_UPPER", 1), ("SMFV_TRSM_UNIT_DIAG", 2), ("SMFV_TRSM_NO_CHAIN", 4),
                         ("SMFV_TRSM_CHAIN_ALL", 8), ("SMFV_TRSM_STATS", 12), ("SMFV_PLAN_STATS", 18)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src), macro
    assert "smfv_csr_transpose" in src[src.index("triangular solves"):src.index("SMFV_TRSM_UPPER 1")]  # T^T: said so
    from sparsematrixmultiplicationmpi_amd import _lib as binding, engine
    assert (engine.TRSM_UPPER, engine.TRSM_UNIT_DIAG, engine.TRSM_NO_CHAIN, engine.TRSM_CHAIN_ALL) == (1, 2, 4, 8)
    assert engine.TRSM_STATS == 12 == len(engine.TRSM_STAT_NAMES)
    assert set(names) <= set(binding.exported_symbols())


def test_trsm_python_surface_without_device():
    """What needs no device: flags, the host analysis, and refusals that come before any library call."""
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import engine
    assert callable(smfv.sptrsm) and callable(smfv.TrsmPlan) and hasattr(smfv.DeviceCSR, "trsm_plan")
    assert engine.trsm_flags("upper", True, "all") == 1 | 2 | 8 and engine.trsm_flags(chain="off", thin_rows=5) == 4 | 5 << 8
    for kw in ({"uplo": "diagonal"}, {"chain": "maybe"}, {"thin_rows": 1 << 16}):
        with pytest.raises(ValueError):
            smfv.TrsmPlan(None, 32, **kw)
    A = T.band()
    S = smfv.SparseMatrix(A.values, A.colIndices, A.rowPtr, A.numRows, A.numCols)
    st = smfv.trsm_analyse(S, 32, "upper", chain="off")
    assert st["levels"] == st["launches"] == 946 and st["chain_launches"] == 0 and st["plan_bytes"] == 0
    with pytest.raises(smfv.SmfvError, match="K = 0"):
        smfv.trsm_analyse(S, 0)


def test_trsm_kernel_notes(tmp_path):
    """The new kernels' code-object notes: every instance of k_trsm_level,
    k_trsm_chain and k_trsm_diag is there, with no spills, no scratch and no
    LDS.  At most 128 VGPRs: a 1024-lane chain block is 4 waves per SIMD and
    cannot launch with more, and the level kernel then keeps at least 4 waves
    per SIMD, each lane with up to 8 gathers in flight."""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no ROCm llvm tools")
    notes = _kernel_notes(tmp_path)
    for kernel, instances, vmax in (("k_trsm_level", 28, 128), ("k_trsm_chain", 28, 128), ("k_trsm_diag", 1, 128)):
        mine = {k: v for k, v in notes.items() if re.match(rf"_ZN4smfv\d+{kernel}[EI]", k)}
        assert len(mine) == instances, (kernel, sorted(mine))
        for name, (vgpr, vspill, sspill, lds, scratch) in mine.items():
            assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0 and vgpr <= vmax, (name, mine[name])


def test_trsm_sanitized_standalone(tmp_path):
    """smfv::build_trsm_plan / trsm_levels under AddressSanitizer + UBSan in a
    stand-alone program (tests/cpp/trsm_check.cpp, its own main); exit 0 and
    no sanitizer report."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "trsm_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                            "-static-libasan",  # the runtime inside the program: it needs nothing from its environment
                            "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "trsm_check.cpp"),
                            os.path.join(CSRC, "smfv_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "trsm_check: OK" in run.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in run.stderr, run.stderr[-3000:]
