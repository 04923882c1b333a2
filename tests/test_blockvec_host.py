"""Host-side checks of the block-vector family (smfv_coldot_*, smfv_col_axpy_f64,
smfv_col_xpay_f64, smfv_pcg_update_f64, BlockPCG): the two reference forms of
the column-dot rule against each other, the guard that the test inputs tell a
wrong summation order apart, smfv_coldot_host against the reference, the pinned
constants, every refusal before any device call, the Python surface that needs
no device, the code-object notes of the new kernels and a sanitizer build of
the host code as a stand-alone program.  No GPU.
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
import blockvec_ref as BR  # noqa: E402
from test_transpose_host import _kernel_notes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsematrixmultiplicationmpi_amd")
CSRC = os.path.join(PKG, "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
SMFV_ERR_INVALID = -1
MS = (0, 1, 31, 32, 33, 511, 512, 513, 1025, 5000)
KS = (1, 3, 32, 40)
VP, I64, CI = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def _lib():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    lib.smfv_last_error.restype = ctypes.c_char_p
    lib.smfv_coldot_rule.argtypes = [ctypes.POINTER(CI), ctypes.POINTER(CI)]
    lib.smfv_coldot_workspace_bytes.argtypes = [CI, CI, ctypes.POINTER(ctypes.c_size_t)]
    lib.smfv_coldot_host.argtypes = [CI, CI, VP, I64, VP, I64, VP]
    lib.smfv_coldot_f64.argtypes = [CI, CI, VP, I64, VP, I64, VP, VP, VP]
    for name in ("smfv_col_axpy_f64", "smfv_col_xpay_f64"):
        getattr(lib, name).argtypes = [CI, CI, VP, VP, CI, VP, I64, VP, I64, VP]
    lib.smfv_pcg_update_f64.argtypes = [CI, CI, VP, VP, CI, VP, I64, VP, I64, VP, I64, VP, I64, VP, VP, VP]
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(bits(a[~np.isnan(b)]), bits(b[~np.isnan(b)]))


def uniform(m, K, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (m, K))


def host_coldot(lib, X, Y, ldx=None, ldy=None):
    """smfv_coldot_host on X, Y placed in NaN-padded arrays of leading dimension ldx / ldy."""
    m, K = X.shape
    ldx, ldy = ldx or K, ldy or K
    Xp, Yp = np.full((m, ldx), np.nan), np.full((m, ldy), np.nan)
    Xp[:, :K], Yp[:, :K] = X, Y
    out = np.full(K + 2, np.nan)
    rc = lib.smfv_coldot_host(m, K, Xp.ctypes.data, ldx, Yp.ctypes.data, ldy, out.ctypes.data)
    assert rc == 0, lib.smfv_last_error()
    assert np.isnan(out[K:]).all()
    return out[:K]


def special_blocks():
    """The special-value block of tests/test_gpu_blockvec.py, built here too
    (the host tests import nothing that needs torch)."""
    m, K = 1100, 12
    X, Y = uniform(m, K, 7), uniform(m, K, 8)
    inf = np.inf
    X[5, 0] = np.nan
    X[40, 1], Y[40, 1] = inf, 2.0
    X[700, 2], Y[700, 2] = -inf, 3.0
    X[9, 3], Y[9, 3] = inf, 0.0
    X[0, 4], Y[0, 4], X[1, 4], Y[1, 4] = inf, 1.0, -inf, 1.0
    X[0, 5], Y[0, 5], X[600, 5], Y[600, 5] = inf, 1.0, -inf, 1.0
    X[:, 6], Y[:, 6] = X[:, 6] * 1e-160, Y[:, 6] * 1e-160
    X[77, 7], Y[77, 7] = 2.0 ** 600, 2.0 ** 600
    X[:, 8], Y[:, 8] = X[:, 8] * 2.0 ** 600, Y[:, 8] * 2.0 ** -600
    X[:, 9], Y[:, 9] = 0.0, 1.0
    X[0, 9], X[32, 9], Y[32, 9] = 0.75, 0.75, -1.0
    X[:, 10], Y[:, 10] = -1.0, 0.0
    X[:, 11], Y[:, 11] = X[:, 11] * 2.0 ** -600, Y[:, 11] * 2.0 ** -600
    return X, Y


@pytest.mark.parametrize("m", [0, 1, 31, 32, 33, 511, 512, 513, 1025, 1500])
def test_reference_forms_agree(m):
    """The vectorised form and the plain loops of the rule agree bit for bit."""
    X, Y = uniform(m, 5, m), uniform(m, 5, m + 1)
    assert same_bits(BR.coldot(X, Y), BR.coldot_loops(X, Y))
    assert same_bits(BR.coldot(X, X), BR.coldot_loops(X, X))


def test_reference_forms_agree_special():
    X, Y = special_blocks()
    assert same_bits(BR.coldot(X, Y), BR.coldot_loops(X, Y))


@pytest.mark.parametrize("m", [m for m in MS if m >= 31])
def test_inputs_tell_orders_apart(m):
    """On the test inputs the rule's result differs from the row-sequential
    sum and from np.sum in at least one column: a wrong order cannot pass."""
    for K in KS:
        if K < 3:
            continue
        X, Y = uniform(m, K, 1000 * m + K), uniform(m, K, 1000 * m + K + 500)
        want = BR.coldot(X, Y)
        assert not np.array_equal(bits(want), bits(BR.rowseq_dot(X, Y))), K
        assert not np.array_equal(bits(want), bits((X * Y).sum(0))), K
        np.testing.assert_allclose(want, (X * Y).sum(0), rtol=0, atol=1e-12 * max(m, 1))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("m", MS)
def test_coldot_host_matches_reference(m, K):
    """smfv_coldot_host against the reference: contiguous, padded leading
    dimensions (the padding is NaN: reading it would show), X is Y."""
    lib = _lib()
    X, Y = uniform(m, K, 1000 * m + K), uniform(m, K, 1000 * m + K + 500)
    want = BR.coldot(X, Y)
    assert same_bits(host_coldot(lib, X, Y), want)
    assert same_bits(host_coldot(lib, X, Y, K + 3, K + 1), want)
    got = host_coldot(lib, X, X, K + 2, K + 2)
    assert same_bits(got, BR.coldot(X, X)) and not np.signbit(got).any()
    if m == 0:
        assert np.array_equal(bits(got), np.zeros(K, np.int64))


def test_coldot_host_special_values():
    """NaN gives NaN, +-inf, inf * 0 and inf - inf (across strands, across
    chunks) give NaN, subnormal products, 2^+-600, a column cancelling to
    exactly +0.0 and a column of -0.0 products giving +0.0."""
    lib = _lib()
    X, Y = special_blocks()
    want = BR.coldot(X, Y)
    assert np.isnan(want[[0, 3, 4, 5]]).all() and want[1] == np.inf and want[2] == -np.inf and want[7] == np.inf
    assert 0 < want[6] < 2.3e-308 and np.isfinite(want[8]) and want[8] != 0
    assert np.array_equal(bits(want[[9, 10, 11]]), [0, 0, 0])
    assert same_bits(host_coldot(lib, X, Y), want)
    assert same_bits(host_coldot(lib, X, Y, 15, 13), want)


def test_rule_constants_pinned():
    """CHUNK = 512 and STRANDS = 32 are the contract; the workspace is
    max(1, chunks) * K doubles."""
    lib = _lib()
    chunk, strands = CI(-1), CI(-1)
    assert lib.smfv_coldot_rule(ctypes.byref(chunk), ctypes.byref(strands)) == 0
    assert (chunk.value, strands.value) == (512, 32) == (BR.CHUNK, BR.STRANDS)
    assert lib.smfv_coldot_rule(None, ctypes.byref(strands)) == SMFV_ERR_INVALID
    b = ctypes.c_size_t(7)
    for m, K, want in ((0, 1, 8), (1, 1, 8), (512, 32, 256), (513, 32, 512), (121192, 32, 237 * 256), (2 ** 31 - 1, 128, 4194304 * 1024)):
        assert lib.smfv_coldot_workspace_bytes(m, K, ctypes.byref(b)) == 0 and b.value == want, (m, K, b.value)
    for m, K in ((-1, 4), (4, 0)):
        assert lib.smfv_coldot_workspace_bytes(m, K, ctypes.byref(b)) == SMFV_ERR_INVALID
    assert lib.smfv_coldot_workspace_bytes(4, 4, None) == SMFV_ERR_INVALID
    with open(os.path.join(ROOT, "include", "smfv.h")) as f:
        src = f.read()
    for macro, value in (("SMFV_COL_NEGATE", 1), ("SMFV_COL_ZERO_DEN", 2)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", src), macro
    text = src[src.index("Block vectors: column dots"):src.index("#define SMFV_COL_NEGATE")]
    for word in ("CHUNK = 512", "STRANDS = 32", "h = 16, 8, 4, 2, 1", "ascending chunk", "never becomes -0.0", "Out of scope",
                 "true IEEE division", "bit-identical", "before any device call"):
        assert word in text, word


def test_refusals_before_any_device_call():
    """Every device entry answers SMFV_ERR_INVALID -- not a HIP error, which is
    what a device call gives where there is no device -- with a message.  The
    pointers are host arrays: a launch would not get as far as using them."""
    lib = _lib()
    m, K = 20, 8
    a, b, c, d = (np.zeros(4096) for _ in range(4))
    s = np.zeros(64)
    A, B, C, D, S = (x.ctypes.data for x in (a, b, c, d, s))

    def refused(rc, word):
        msg = lib.smfv_last_error().decode()
        assert rc == SMFV_ERR_INVALID and word in msg, (rc, word, msg)

    dot = lib.smfv_coldot_f64
    refused(dot(m, 0, A, K, B, K, S, S, None), "K = 0")
    refused(dot(-1, K, A, K, B, K, S, S, None), "m = -1")
    refused(dot(m, K, A, K - 1, B, K, S, S, None), "leading dimension of X")
    refused(dot(m, K, A, K, B, K - 1, S, S, None), "leading dimension of Y")
    refused(dot(m, K, None, K, B, K, S, S, None), "null X")
    refused(dot(m, K, A, K, None, K, S, S, None), "null Y")
    refused(dot(m, K, A, K, B, K, None, S, None), "null out")
    refused(dot(m, K, A, K, B, K, S, None, None), "null workspace")
    refused(lib.smfv_coldot_host(m, K, A, K, B, K, None), "null out")
    refused(lib.smfv_coldot_host(m, K, A, 2, B, K, S), "leading dimension of X")
    for name in ("smfv_col_axpy_f64", "smfv_col_xpay_f64"):
        fn, tag = getattr(lib, name), name[5:-4]
        refused(fn(m, 0, S, S, 0, A, K, B, K, None), tag + ": K = 0")
        refused(fn(-2, K, S, S, 0, A, K, B, K, None), "m = -2")
        refused(fn(m, K, None, S, 0, A, K, B, K, None), "null num")
        refused(fn(m, K, S, None, 4, A, K, B, K, None), "unknown flags 4")
        refused(fn(m, K, S, None, 0, None, K, B, K, None), "null X")
        refused(fn(m, K, S, None, 0, A, K, None, K, None), "null Y")
        refused(fn(m, K, S, None, 0, A, K, B, K - 1, None), "leading dimension of Y")
    upd = lib.smfv_pcg_update_f64
    refused(upd(m, K, S, S, 0, A, K, B, K, C, K, C, K, S, S, None), "X and R overlap")
    refused(upd(m, K, S, S, 0, A, K, A, K, C, K, D, K, S, S, None), "P and Q overlap")
    refused(upd(m, K, S, S, 0, A, K, B, K, C, K, C + 8 * 3 * K, K, S, S, None), "X and R overlap")
    refused(upd(m, K, S, S, 0, A, K, A + 40, K, C, K, D, K, S, S, None), "P and Q overlap")
    refused(upd(m, K, S, S, 0, A, 2 * K, B, K, C, K, A + 8 * (K - 1), 2 * K, S, S, None), "P and R overlap")
    refused(upd(m, K, S, S, 0, None, K, B, K, C, K, D, K, S, S, None), "null P")
    refused(upd(m, K, None, S, 0, A, K, B, K, C, K, D, K, S, S, None), "null num")
    refused(upd(m, K, S, S, 0, A, K, B, K, C, K, D, K, None, S, None), "null rr")
    refused(upd(m, K, S, S, 0, A, K, B, K, C, K, D, K, S, None, None), "null workspace")
    refused(upd(m, K, S, S, 16, A, K, B, K, C, K, D, K, S, S, None), "unknown flags")
    refused(upd(m, K, S, S, 0, A, K, B, K, C, K - 1, D, K, S, S, None), "leading dimension of X")
    refused(upd(m, 0, S, S, 0, A, K, B, K, C, K, D, K, S, S, None), "K = 0")
    assert not a.any() and not c.any() and not s.any()


def test_python_surface_without_device():
    """Imports, names, constants and signatures; nothing here touches a device."""
    import inspect
    import sparsematrixmultiplicationmpi_amd as smfv
    from sparsematrixmultiplicationmpi_amd import _lib as binding, engine
    names = ("smfv_coldot_rule", "smfv_coldot_workspace_bytes", "smfv_coldot_host", "smfv_coldot_f64", "smfv_col_axpy_f64",
             "smfv_col_xpay_f64", "smfv_pcg_update_f64")
    assert set(names) <= set(binding.exported_symbols())
    for fn in ("coldot", "col_axpy", "col_xpay", "pcg_update", "coldot_rule", "BlockPCG"):
        assert callable(getattr(smfv, fn)), fn
    assert smfv.coldot_rule() == (512, 32)
    assert (engine.COL_NEGATE, engine.COL_ZERO_DEN) == (1, 2)
    assert engine.coldot_workspace_doubles(513, 32) == 64 and engine.coldot_workspace_doubles(0, 3) == 3
    for attr in ("start", "iterate", "solve", "residuals", "rr", "bb"):
        assert hasattr(smfv.BlockPCG, attr), attr
    sig = inspect.signature(smfv.BlockPCG.solve).parameters
    assert (sig["tol"].default, sig["check_every"].default, sig["graph"].default, sig["X0"].default) == (1e-8, 1, False, None)
    assert inspect.signature(smfv.BlockPCG).parameters["M"].default is None
    assert list(inspect.signature(smfv.coldot).parameters)[:4] == ["X", "Y", "out", "stream"]


def test_kernel_notes(tmp_path):
    """The code-object notes of the new kernels: every instance (7 team widths
    x 8- / 16-byte accesses) has no spills and no scratch; the elementwise
    kernels and k_coldot_final use no LDS; the chunk kernels use exactly the
    256 values the tree needs across wavefronts, and none where a chunk's
    strands share a wavefront (team widths 1 and 2); no other kernel of these
    names exists."""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no ROCm llvm tools")
    notes = _kernel_notes(tmp_path)
    new = {k: v for k, v in notes.items() if re.search(r"coldot|col_axpy|col_xpay|pcg_update", k)}
    seen = set()
    for kernel, tree in (("k_coldot_partial", True), ("k_pcg_update", True), ("k_col_axpy", False), ("k_col_xpay", False)):
        mine = {k: v for k, v in new.items() if re.match(rf"_ZN4smfv\d+{kernel}ILi(\d+)ELi([12])EEE", k)}
        assert len(mine) == 14, (kernel, sorted(mine))
        for name, (vgpr, vspill, sspill, lds, scratch) in mine.items():
            team, vec = map(int, re.match(rf"_ZN4smfv\d+{kernel}ILi(\d+)ELi([12])EEE", name).groups())
            assert vspill == 0 and sspill == 0 and scratch == 0, (name, mine[name])
            assert lds == (256 * 8 * vec if tree and team >= 4 else 0), (name, lds)
            if not tree:
                assert vgpr <= 128, (name, vgpr)  # four waves per SIMD at the least
        seen |= set(mine)
    final = [k for k in new if re.match(r"_ZN4smfv\d+k_coldot_finalE", k)]
    assert len(final) == 1 and notes[final[0]][1:] == (0, 0, 0, 0), final
    seen.add(final[0])
    assert set(new) == seen, sorted(set(new) - seen)


def test_blockvec_sanitized_standalone(tmp_path):
    """smfv::coldot_host and the argument checks under AddressSanitizer + UBSan
    in a stand-alone program (tests/cpp/blockvec_check.cpp, its own main); exit
    0 and no sanitizer report."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "blockvec_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                            "-static-libasan",  # the runtime inside the program: it needs nothing from its environment
                            "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "blockvec_check.cpp"),
                            os.path.join(CSRC, "smfv_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "blockvec_check: OK" in run.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert word not in run.stderr, run.stderr[-3000:]
