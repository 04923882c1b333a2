"""Host-side checks of ILU(0) (smfv_ilu0_*): a guard on the numpy reference
itself (the LU backward bound on the pattern positions), the library's analysis
figures against numpy's recounts and trsm_ref.schedule on every input, the
refusals, symbols and constants, the Python surface that needs no device, the
code-object notes of the new kernels and a sanitizer build of the host
analysis as a stand-alone program.  No GPU.
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
import ilu0_ref as R  # noqa: E402
import trsm_ref as T  # noqa: E402
from test_transpose_host import _kernel_notes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsematrixmultiplicationmpi_amd")
CSRC = os.path.join(PKG, "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
SMFV_ERR_INVALID = -1
IP = ctypes.POINTER(ctypes.c_int)
PD = ctypes.POINTER(ctypes.c_double)
NO_CHAIN, CHAIN_ALL, NSTATS = 4, 8, 15
NAMES = ("band", "grid9", "long_row", "wide", "special") + R.DEGENERATE


def _input(name):
    return R.special()[0] if name == "special" else R.INPUTS[name]()


def _lib():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    lib.smfv_ilu0_analyse.restype = ctypes.c_int
    lib.smfv_ilu0_analyse.argtypes = [ctypes.c_int, IP, IP, ctypes.c_int, PD]
    lib.smfv_ilu0_plan_create.restype = ctypes.c_int
    lib.smfv_ilu0_plan_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int64, IP, IP, ctypes.c_int]
    lib.smfv_last_error.restype = ctypes.c_char_p
    return lib


def _analyse(lib, A, flags, ci=None, rp=None):
    rp = np.ascontiguousarray(A.rowPtr if rp is None else rp, np.int32)
    ci = np.ascontiguousarray(A.colIndices if ci is None else ci, np.int32)
    out = np.full(NSTATS, -7.0)
    rc = lib.smfv_ilu0_analyse(A.numRows, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), flags, out.ctypes.data_as(PD))
    return rc, out


def test_input_facts():
    """What the inputs are for, against the figures the cases were designed with."""
    A, f = R.reference("band")
    c = R.counts(A)
    lev = T.levels(A)
    assert (A.nnz, c["steps"], c["pairs"], int(lev.max()), int(np.diff(A.rowPtr).max())) == (62137, 29604, 99230, 953, 41)
    assert np.isfinite(f).all() and 24.0 < np.abs(f).max() < 25.0
    unsorted = sum(bool(np.any(np.diff(A.colIndices[A.rowPtr[i]:A.rowPtr[i + 1]]) < 0)) for i in range(A.numRows))
    assert unsorted > 1000
    A, f = R.reference("grid9")
    c = R.counts(A)
    assert A.numRows == 576 and (c["steps"], c["pairs"]) == (2162, 6394) and np.isfinite(f).all()
    w = np.bincount(T.levels(A))[1:]
    assert w.max() > 8 * np.median(np.bincount(T.levels(R.band()))[1:]) / 3  # wide where band is thin
    A, _ = R.reference("long_row")
    c = R.counts(A)
    assert c["max_steps"] == 2999 > R.SLOT and c["long_rows"] == 1 and int(T.levels(A).max()) == 3000
    A, _ = R.reference("wide")
    w = np.bincount(T.levels(A))[1:]
    assert w.tolist() == [375] * 8 and R.counts(A)["max_pairs"] == 28
    for case in ("diagonal", "upper_bidiagonal"):
        A, f = R.reference(case)
        assert R.counts(A)["steps"] == 0 and int(T.levels(A).max()) == 1
        assert np.array_equal(f.view(np.uint64), np.asarray(A.values).view(np.uint64))  # every row copied
    A, f = R.reference("special")
    _, info = R.special()
    assert 0.8 <= np.isfinite(f).mean() < 1.0 and np.isnan(f).any() and np.isinf(f).any()
    first_bad = np.repeat(np.arange(A.numRows), np.diff(A.rowPtr))[~np.isfinite(f)].min()
    assert first_bad >= A.numRows - 150
    zeros = f[f == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert not np.array_equal(R.reference("band2")[1], R.reference("band")[1])


@pytest.mark.parametrize("name", ["band", "grid9"])
def test_reference_guard(name):
    """|A - L U|_ij <= gamma_n (|L| |U|)_ij on every pattern entry, n = the
    row's steps + 1, gamma_n = n u / (1 - n u), u = 2^-53: the standard LU
    backward bound at the pattern positions, where ILU(0) is exact LU.  The
    products are summed in np.longdouble.  Measured by this test, whose sums are
    in np.longdouble so that the check adds no rounding of its own: the largest
    ratio to the bound is 0.46 on `band` and 0.56 on `grid9`.  (An earlier CPU check of the
    same bound on these inputs gave 0.67 and 0.76; how it summed the products is
    not recorded, and a sum in fp64 adds rounding of the bound's own size.  Both
    pairs lie under 1, which is what is asserted.)"""
    A, f = R.reference(name)
    m, rp, ci = A.numRows, A.rowPtr, A.colIndices
    a = np.asarray(A.values)
    LD = np.longdouble
    u = LD(2.0) ** -53
    worst = 0.0
    for i in range(m):
        s, e = int(rp[i]), int(rp[i + 1])
        cols = ci[s:e].tolist()
        pos = {c: t for t, c in enumerate(cols)}
        lu = np.zeros(e - s, LD)
        ab = np.zeros(e - s, LD)
        nsteps = 0
        for t, k in enumerate(cols):
            if k > i:
                continue
            l = LD(1.0) if k == i else LD(f[s + t])  # L's unit diagonal
            nsteps += k < i
            for q in range(int(rp[k]), int(rp[k + 1])):
                c = int(ci[q])
                if c >= k and c in pos:
                    lu[pos[c]] += l * LD(f[q])
                    ab[pos[c]] += abs(l) * abs(LD(f[q]))
        n = nsteps + 1
        gamma = n * u / (1 - n * u)
        err = np.abs(a[s:e].astype(LD) - lu)
        assert np.all(err <= gamma * ab), (name, i)
        worst = max(worst, float(np.max(err / (gamma * ab))))
    print("ILU0 reference guard", name, "largest ratio to the bound", round(worst, 3))
    assert worst > 0.0


@pytest.mark.parametrize("chain,thin", [("auto", 0), ("off", 0), ("all", 0), ("auto", 3)])
@pytest.mark.parametrize("name", NAMES)
def test_analyse_matches_numpy(name, chain, thin):
    A = _input(name)
    flags = {"auto": 0, "off": NO_CHAIN, "all": CHAIN_ALL}[chain] | thin << 8
    rc, out = _analyse(_lib(), A, flags)
    assert rc == 0, _lib().smfv_last_error()
    lev = R.levels(name)
    w = np.bincount(lev)[1:] if lev.size else np.zeros(1, np.int64)
    assert int(out[14]) == (thin or 64)  # the solves' default
    launches, chains, rows, most = T.schedule(lev, int(out[14]), chain)
    c = R.counts_of(name)
    assert [int(v) for v in out[:12]] == [int(lev.max()) if lev.size else 0, int(w.max()), launches, chains, rows, most,
                                          c["steps"], c["pairs"], c["max_steps"], c["max_pairs"], c["long_rows"], R.SLOT]
    assert out[12] == 0 and out[13] >= 0
    if chain == "off":
        assert launches == (int(lev.max()) if lev.size else 0) and chains == 0
    if chain == "all" and lev.size:
        assert launches == 1 and rows == A.numRows


def _refusal_cases():
    A = R.band()
    m = A.numRows
    r = np.repeat(np.arange(m), np.diff(A.rowPtr))
    no_diag = A.colIndices.copy()
    for row in (1711, 99):  # the diagonal entry of these rows becomes a column their row lacks
        s, e = A.rowPtr[row], A.rowPtr[row + 1]
        free = next(c for c in range(row + 1, m) if c not in A.colIndices[s:e])
        no_diag[(r == row) & (no_diag == row)] = free
    dup = A.colIndices.copy()
    j1, j2 = [j for j in range(int(A.rowPtr[200]), int(A.rowPtr[201])) if A.colIndices[j] != 200][:2]
    dup[j2] = dup[j1]  # two entries of row 200 in one column, its diagonal entry kept
    dupcol = int(dup[j1])
    bad_col = A.colIndices.copy()
    bad_col[7] = m
    rp_start, rp_down = np.array(A.rowPtr), np.array(A.rowPtr)
    rp_start[0] = 1
    rp_down[500] = rp_down[499] - 1
    return A, [(no_diag, None, 0, ("row 99 ", "diagonal")), (dup, None, 0, ("row 200 ", f"column {dupcol} ")),
               (bad_col, None, 0, ("column index 3000 ",)), (None, rp_start, 0, ("row_ptr[0]",)),
               (None, rp_down, 0, ("row_ptr decreases",)), (None, None, 1 << 28, ("unknown flags",)),
               (None, None, 3, ("unknown flags",)), (None, None, NO_CHAIN | CHAIN_ALL, ("NO_CHAIN", "CHAIN_ALL"))]


def test_refusals():
    lib = _lib()
    A, cases = _refusal_cases()
    for ci, rp, flags, words in cases:
        rc, out = _analyse(lib, A, flags, ci, rp)
        msg = lib.smfv_last_error().decode()
        assert rc == SMFV_ERR_INVALID and (out == -7).all(), (words, rc)
        assert msg.startswith("ilu0") and all(w in msg for w in words), msg
    assert _analyse(lib, T.band(), 0)[0] == SMFV_ERR_INVALID  # trsm's band: duplicated diagonals
    assert "more than once" in lib.smfv_last_error().decode()


def test_create_refuses_before_any_device_call():
    """smfv_ilu0_plan_create answers SMFV_ERR_INVALID -- not a HIP error, which
    is what a device call would give where there is no device -- and makes no
    plan: everything is checked on the host first."""
    lib = _lib()
    A, cases = _refusal_cases()
    for ci, rp, flags, words in cases:
        h = ctypes.c_void_p()
        rp = np.ascontiguousarray(A.rowPtr if rp is None else rp, np.int32)
        ci = np.ascontiguousarray(A.colIndices if ci is None else ci, np.int32)
        rc = lib.smfv_ilu0_plan_create(ctypes.byref(h), A.numRows, A.nnz, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), flags)
        assert rc == SMFV_ERR_INVALID and not h.value and all(w in lib.smfv_last_error().decode() for w in words), words


def test_ilu0_symbols_and_constants():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    names = ("smfv_ilu0_plan_create", "smfv_ilu0_plan_factor", "smfv_ilu0_plan_stats", "smfv_ilu0_plan_destroy",
             "smfv_ilu0_analyse")
    for name in names:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "smfv.h")) as f:
        src = f.read()
    for macro, value in (("SMFV_ILU0_NO_CHAIN", 4), ("SMFV_ILU0_CHAIN_ALL", 8), ("SMFV_ILU0_STATS", 15),
                         ("SMFV_TRSM_STATS", 12), ("SMFV_PLAN_STATS", 18)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src), macro
    assert re.search(r"#define\s+SMFV_ILU0_THIN_ROWS\(r\)\s+\(\(\(r\) & 0xffff\) << 8\)", src)
    text = src[src.index("ILU(0): the factors"):src.index("SMFV_ILU0_NO_CHAIN 4")]
    assert "Out of scope" in text and "IC(0)" in text and "never an FMA" in text
    from sparsematrixmultiplicationmpi_amd import _lib as binding, engine
    assert (engine.ILU0_NO_CHAIN, engine.ILU0_CHAIN_ALL) == (4, 8)
    assert engine.ILU0_STATS == 15 == len(engine.ILU0_STAT_NAMES)
    assert set(names) <= set(binding.exported_symbols())


def test_ilu0_python_surface_without_device():
    """What needs no device: flags, the host analysis, and refusals that come before any library call."""
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import engine
    assert callable(smfv.ilu0) and callable(smfv.Ilu0Plan) and callable(smfv.Ilu0Preconditioner)
    assert hasattr(smfv.DeviceCSR, "ilu0_plan") and hasattr(smfv.DeviceCSR, "like")
    assert engine.ilu0_flags("all") == 8 and engine.ilu0_flags(chain="off", thin_rows=5) == 4 | 5 << 8
    assert engine.ilu0_flags() == 0
    for kw in ({"chain": "maybe"}, {"thin_rows": 1 << 16}, {"thin_rows": -1}):
        with pytest.raises(ValueError):
            smfv.Ilu0Plan(None, **kw)
    A = R.band()
    S = smfv.SparseMatrix(A.values, A.colIndices, A.rowPtr, A.numRows, A.numCols)
    st = smfv.ilu0_analyse(S, chain="off")
    assert st["levels"] == st["launches"] == 953 and st["chain_launches"] == 0 and st["plan_bytes"] == 0
    assert (st["steps"], st["pairs"], st["lds_slot_entries"]) == (29604, 99230, 256)
    B = T.band()
    with pytest.raises(smfv.SmfvError, match="more than once"):
        smfv.ilu0_analyse(smfv.SparseMatrix(B.values, B.colIndices, B.rowPtr, B.numRows, B.numCols))


def test_ilu0_kernel_notes(tmp_path):
    """The new kernels' code-object notes: k_ilu0_level and k_ilu0_chain are
    there, one instance each, with no spills, no scratch, at most 128 VGPRs (a
    1024-lane block cannot launch with more) and the static LDS the header
    states: a slot of 256 doubles per wavefront, 8,192 and 32,768 bytes."""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no ROCm llvm tools")
    notes = _kernel_notes(tmp_path)
    with open(os.path.join(ROOT, "include", "smfv.h")) as f:
        src = f.read()
    assert "256 doubles of LDS: 8,192 bytes" in src and "32,768\n * bytes of LDS" in src
    for kernel, lds_bytes in (("k_ilu0_level", 8192), ("k_ilu0_chain", 32768)):
        mine = {k: v for k, v in notes.items() if re.match(rf"_ZN4smfv\d+{kernel}E", k)}
        assert len(mine) == 1, (kernel, sorted(mine))
        for name, (vgpr, vspill, sspill, lds, scratch) in mine.items():
            assert vspill == 0 and sspill == 0 and scratch == 0 and lds == lds_bytes and vgpr <= 128, (name, mine[name])
    assert not [k for k in notes if "k_ilu0" in k and not re.match(r"_ZN4smfv\d+k_ilu0_(level|chain)E", k)]


def test_ilu0_sanitized_standalone(tmp_path):
    """smfv::build_ilu0_plan under AddressSanitizer + UBSan in a stand-alone
    program (tests/cpp/ilu0_check.cpp, its own main); exit 0 and no sanitizer
    report."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "ilu0_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                            "-static-libasan",  # the runtime inside the program: it needs nothing from its environment
                            "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ilu0_check.cpp"),
                            os.path.join(CSRC, "smfv_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "ilu0_check: OK" in run.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in run.stderr, run.stderr[-3000:]
