"""Device-side SpMM: Y = A_csr * X on an MI355X through the libsmfv C ABI.

Python mirror of the reference's hot-path call surface
(SC = /root/reference/Source Code):

    sparseMatrixFatVectorMultiply              SC/SparseMatrixFatVectorMultiply.h:14-15
    sparseMatrixFatVectorMultiplyRowWise       SC/SparseMatrixFatVectorMultiplyRowWise.h:15-17
    sparseMatrixFatVectorMultiplyColumnWise    SC/SparseMatrixFatVectorMultiplyColumnWise.h:15
    sparseMatrixFatVectorMultiplyNonZeroElement SC/SparseMatrixFatVectorMultiplyNonZeroElement.h:15

Same arguments (A, fat vector, vecCols) and result (m x K, row-major).  The
MPI variants are collective over a Communicator (dist.py) when one is given
and return the result on rank 0 only (an empty (0, K) array elsewhere), as
SC/...RowWise.cpp:125 does; without one they run on the local GPU.

torch is used only for device memory and the current HIP stream.  Every
compute call goes to the HIP kernels; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_size_t
from enum import IntEnum

import numpy as np
import torch

from ._lib import call
from .inputs import SparseMatrix, csr_permute_pattern, multicolor_order_pattern


class Variant(IntEnum):
    SEQUENTIAL = 0   # SC/SparseMatrixFatVectorMultiply.cpp:11-31
    ROWWISE = 1      # SC/SparseMatrixFatVectorMultiplyRowWise.cpp:12-126
    COLUMNWISE = 2   # SC/SparseMatrixFatVectorMultiplyColumnWise.cpp:13-131
    NONZERO = 3      # SC/SparseMatrixFatVectorMultiplyNonZeroElement.cpp:12-120


def _require_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("smfv: no HIP device visible; the SpMM engine has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def stream_handle(stream: torch.cuda.Stream | None = None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


class DeviceCSR:
    """A CSR matrix resident in HBM (int32 row_ptr / col_idx, f64 values)
    plus the host copy of the pattern the plans analyse.

    spmm() keeps one plan per (variant, K) on the matrix (analysed once).  A
    tiled plan computes with a snapshot of the values taken when it was bound
    (include/smfv.h, values contract).  The cached plans re-bind by
    themselves when `values` has changed since their bind -- a new tensor, or
    an in-place change (torch's version counter of the tensor) -- and
    values_changed() re-binds them explicitly (e.g. after a write torch did
    not see, such as a kernel of another library)."""

    def __init__(self, A: SparseMatrix, device: torch.device | None = None):
        device = device or _require_device()
        A.validate()
        self.m, self.n, self.nnz = A.numRows, A.numCols, A.nnz
        self.h_row_ptr = np.ascontiguousarray(A.rowPtr, dtype=np.int32)
        self.h_col_idx = np.ascontiguousarray(A.colIndices, dtype=np.int32)  # plan analysis
        self.row_ptr = torch.from_numpy(self.h_row_ptr).to(device)
        self.col_idx = torch.from_numpy(self.h_col_idx).to(device)
        self.values = torch.from_numpy(np.ascontiguousarray(A.values, dtype=np.float64)).to(device)
        self.device = device
        self._plans: dict = {}

    @property
    def nbytes(self) -> int:
        return 4 * (self.m + 1) + 12 * self.nnz

    def ptrs(self):
        return self.row_ptr.data_ptr(), self.col_idx.data_ptr(), self.values.data_ptr()

    def plan(self, variant: int, K: int, stream: torch.cuda.Stream | None = None,
             transpose: bool = False) -> "SpmmPlan":
        """The cached plan of (variant, K) -- of A, or with `transpose` of A^T
        (Y = A^T X) --, created (and bound on `stream`) on first use."""
        key = (int(variant), int(K), True) if transpose else (int(variant), int(K))
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = SpmmPlan(variant, self, K, stream=stream, transpose=transpose)
        elif p.bound_version != self.values_version():
            p.bind_values(stream)  # values changed since the bind: snapshot them again
        return p

    def trsm_plan(self, K: int, uplo: str = "lower", unit_diag: bool = False, chain: str = "auto",
                  stream: torch.cuda.Stream | None = None) -> "TrsmPlan":
        """The cached triangular-solve plan of (K, uplo, unit_diag, chain),
        created (and bound on `stream`) on first use and bound again when
        `values` has changed since its bind."""
        key = ("trsm", int(K), uplo, bool(unit_diag), chain)
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = TrsmPlan(self, K, uplo, unit_diag, chain, stream=stream)
        elif p.bound_version != self.values_version():
            p.bind_values(stream)
        return p

    def ilu0_plan(self, chain: str = "auto", thin_rows: int = 0) -> "Ilu0Plan":
        """The cached ILU(0) plan of (chain, thin_rows), created on first use.
        It holds no values: every factor() reads `values` as they are then."""
        key = ("ilu0", chain, int(thin_rows))
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = Ilu0Plan(self, chain, thin_rows)
        return p

    def like(self, values: torch.Tensor) -> "DeviceCSR":
        """A DeviceCSR of this pattern with other values: it shares the
        pattern tensors and the host pattern with `self`, and has no plans."""
        if not values.is_cuda or values.dtype != torch.float64 or tuple(values.shape) != (self.nnz,) \
                or not values.is_contiguous():
            raise ValueError(f"values must be a contiguous float64 HIP tensor of {self.nnz} entries")
        B = object.__new__(DeviceCSR)
        B.m, B.n, B.nnz = self.m, self.n, self.nnz
        B.h_row_ptr, B.h_col_idx = self.h_row_ptr, self.h_col_idx
        B.row_ptr, B.col_idx, B.values = self.row_ptr, self.col_idx, values
        B.device = self.device
        B._plans = {}
        return B

    def reordered(self, order="multicolor") -> "ReorderedCSR":
        """This square matrix under another numbering of its rows and columns
        (ReorderedCSR): order="multicolor" (the library's greedy colouring,
        which cuts the levels of the solves and of ILU(0) to the number of
        colours) or an explicit permutation array (new row i is old row
        order[i])."""
        return ReorderedCSR(self, order)

    def values_version(self) -> tuple[int, int]:
        """(address, torch version counter) of `values`: changes with every
        in-place write torch performs and with a new tensor."""
        return self.values.data_ptr(), self.values._version

    def values_changed(self, stream: torch.cuda.Stream | None = None) -> None:
        """Re-bind every cached plan after `values` changed in place."""
        for p in self._plans.values():
            p.bind_values(stream)


def workspace_bytes(variant: int, m: int, nnz: int, K: int) -> int:
    b = c_size_t(0)
    call("smfv_spmm_workspace_bytes", int(variant), m, nnz, K, byref(b))
    return b.value


def _check_dense(T: torch.Tensor, rows: int, K: int, name: str) -> int:
    if not T.is_cuda or T.dtype != torch.float64:
        raise TypeError(f"{name} must be a float64 HIP tensor")
    if T.dim() != 2 or T.shape[0] != rows or T.shape[1] != K:
        raise ValueError(f"{name} must have shape ({rows}, {K}), got {tuple(T.shape)}")
    if K > 0 and T.stride(1) != 1:
        raise ValueError(f"{name} must be row-major (unit column stride)")
    return max(int(T.stride(0)), K)


PLAN_NO_TILES, PLAN_FORCE_TILES, PLAN_FMA, PLAN_NATURAL_SEEDS, PLAN_MFMA, PLAN_SPLIT_ENDS = 1, 2, 4, 8, 16, 32
PLAN_ONE_WAVEFRONT, PLAN_SIMPLE_ROWS, PLAN_CS, PLAN_WS = 64, 128, 256, 512
PLAN_WS_GEOM1, PLAN_WS_GEOM2, PLAN_WS_GEOM3 = 1024, 2048, 4096
PLAN_LIVE_VALUES = 8192  # (r5) the tiled kernel reads the live CSR values (no snapshot, no bind)
PLAN_SINGLE_ROWS = 16384  # (r5) one row per k_rows_ws team (no row pairs; A/B)
PLAN_ROW_PAIRS = 32768  # (r5) row pairs forced (without either: the plan with fewer rounds)
PLAN_AXPBY = 65536  # the plan runs Y = alpha*A*X + beta*Y (smfv_plan_execute_axpby)
PLAN_AXPBY_TWO_PASS = 131072  # ... in the two-pass form (A/B, tests); implies PLAN_AXPBY
PLAN_TRANSPOSE = 262144  # the plan computes Y = A^T X from A's CSR (SMFV_PLAN_TRANSPOSE)
PLAN_STATS = 18  # SMFV_PLAN_STATS
EPILOGUE_MODES = {0: None, 1: "fused", 2: "two_pass"}  # smfv_plan_epilogue_mode
PLAN_KERNELS = {0: None, 1: "k_rows_ws", 2: "k_rows_mfma", 3: "k_spmv_chunks", 5: "k_rows_wsn"}


class SpmmPlan:
    """One variant of Y = A*X analysed once for (A, K) (smfv_plan_create):
    device workspace allocated up front and, for K % 32 == 0 or K = 4 / 8 /
    16 (one narrow column window), the row-tile analysis that lets the kernel
    stage re-used X rows in LDS.  run() is a pure asynchronous launch
    sequence (capturable into a hipGraph).

    tiles: "auto" (stage when re-use >= 3), "off", or "force".  fma: opt-in
    fused multiply-add in the tiled kernel (SMFV_PLAN_FMA).  mfma: opt-in
    dense-block MFMA tiles (SMFV_PLAN_MFMA); the MFMA plan requires a finite
    X, because the dense blocks' zeros multiply every staged X row (an inf or
    NaN in X reaches rows that do not reference it).  rows=(begin,
    end): plan of that row block only (smfv_plan_create_rows; run() writes
    the block's rows to Y[0:end-begin]).  xcd_parts: "auto" (one row range
    per XCD when their X footprints allow it) or "one" (one wavefront cut in
    8 shares; SMFV_PLAN_ONE_WAVEFRONT, A/B).  The values snapshot of a tiled plan
    is gathered on `stream`; a run() on another stream waits for it.
    axpby: True makes the plan runnable with run_axpby() (Y = alpha*A*X +
    beta*Y in place, SMFV_PLAN_AXPBY; the library fuses the epilogue into the
    row kernels' stores where it can: epilogue_mode); "two_pass" forces the
    scratch-and-second-pass form (SMFV_PLAN_AXPBY_TWO_PASS, A/B).
    transpose: True plans Y[A.n x K] = A^T X[A.m x K] (SMFV_PLAN_TRANSPOSE):
    the pattern is transposed once on the host and every other argument acts
    on the transposed pattern; the sums run in A's CSR order per column, so
    the result is bit-identical to the sequential loop on the CSR of A^T.
    Every transposed plan computes from a plan-owned copy of the values in
    transposed order, so it must be bound again whenever the values change
    (untiled and live_values plans too).  Not with rows=."""

    def __init__(self, variant: int, A: DeviceCSR, K: int, tiles: str = "auto", fma: bool = False,
                 stream: torch.cuda.Stream | None = None, rows: tuple[int, int] | None = None,
                 seeds: str = "frontier", mfma: bool = False, split_ends: bool = False,
                 xcd_parts: str = "auto", tiled_kernel: str = "auto", live_values: bool = False,
                 row_pairs: str = "auto", axpby: bool | str = False, transpose: bool = False):
        if transpose and rows is not None:
            raise ValueError("transpose=True has no row-block form (rows=)")
        self.variant, self.A, self.K = Variant(variant), A, K
        self.rows = rows
        self._transposed = bool(transpose)
        flags = {"auto": 0, "off": PLAN_NO_TILES, "force": PLAN_FORCE_TILES}[tiles]
        flags |= {False: 0, True: PLAN_AXPBY, "two_pass": PLAN_AXPBY | PLAN_AXPBY_TWO_PASS}[axpby]
        if live_values:  # (r5) SMFV_PLAN_LIVE_VALUES: value pairs DMA'd from the CSR values, bind a no-op
            flags |= PLAN_LIVE_VALUES
        # (r5) row pairs in k_rows_ws tiles: "auto" (the plan whose busiest
        # block runs fewer tiles), "off" (SMFV_PLAN_SINGLE_ROWS), "on" (SMFV_PLAN_ROW_PAIRS)
        flags |= {"auto": 0, "off": PLAN_SINGLE_ROWS, "on": PLAN_ROW_PAIRS}[row_pairs]
        if fma:  # opt-in fused multiply-add in the tiled kernel: within tolerance, not bit-identical
            flags |= PLAN_FMA
        if seeds == "natural":  # tiles seeded in row order (A/B of the wavefront seeding)
            flags |= PLAN_NATURAL_SEEDS
        if mfma:  # opt-in dense-block MFMA tile kernel: within tolerance, not bit-identical
            flags |= PLAN_MFMA
        if split_ends:  # opt-in: half tiles first and last in every block (A/B; measured slower)
            flags |= PLAN_SPLIT_ENDS
        if {"auto": False, "one": True}[xcd_parts]:
            flags |= PLAN_ONE_WAVEFRONT
        # which tiled kernel for K % 32 == 0: the library's choice, or k_rows_ws
        # (SMFV_PLAN_WS) for A/B; "ws1" / "ws2" / "ws3": k_rows_ws with one
        # 1024-lane / two 512-lane / one 768-lane pipeline(s) per CU
        # (SMFV_PLAN_WS_GEOM1 / 2 / 3)
        flags |= {"auto": 0, "ws": PLAN_WS, "ws1": PLAN_WS | PLAN_WS_GEOM1,
                  "ws2": PLAN_WS | PLAN_WS_GEOM2, "ws3": PLAN_WS | PLAN_WS_GEOM3}[tiled_kernel]
        if transpose:
            flags |= PLAN_TRANSPOSE
        self._plan = ctypes.c_void_p()
        ip = ctypes.POINTER(ctypes.c_int)
        if rows is None:
            call("smfv_plan_create", byref(self._plan), int(variant), A.m, A.n, A.nnz,
                 A.h_row_ptr.ctypes.data_as(ip), A.h_col_idx.ctypes.data_as(ip), K, flags)
            self.m_out = A.n if transpose else A.m
        else:
            r0, r1 = int(rows[0]), int(rows[1])
            call("smfv_plan_create_rows", byref(self._plan), int(variant), r0, r1, A.n,
                 A.h_row_ptr.ctypes.data_as(ip), A.h_col_idx.ctypes.data_as(ip), K, flags)
            self.m_out = r1 - r0
        self.bind_values(stream)

    def bind_values(self, stream: torch.cuda.Stream | None = None) -> None:
        """(Re)bind a tiled plan to A's current device values (after they change)."""
        call("smfv_plan_bind_values", self._plan, self.A.values.data_ptr(), stream_handle(stream))
        self.bound_version = self.A.values_version()

    @property
    def transposed(self) -> bool:
        """True for a plan of Y = A^T X (smfv_plan_is_transposed)."""
        flag = ctypes.c_int(0)
        call("smfv_plan_is_transposed", self._plan, byref(flag))
        return bool(flag.value)

    @property
    def _x_rows(self) -> int:
        return self.A.m if self._transposed else self.A.n

    def stats(self) -> dict:
        out = (ctypes.c_double * PLAN_STATS)()
        call("smfv_plan_stats", self._plan, out)
        return {"tiled": bool(out[0]), "tiles": int(out[1]), "staged_rows": int(out[2]),
                "reuse": float(out[3]), "plan_bytes": int(out[4]), "direct_rows": int(out[5]),
                "row_begin": int(out[6]), "est_reuse": float(out[7]), "analysis_ms": float(out[8]),
                "snapshot_entries": int(out[9]), "mfma": bool(out[10]), "xcd_parts": int(out[11]),
                "footprint": float(out[12]), "kernel": PLAN_KERNELS.get(int(out[13])), "live_values": bool(out[14]),
                "ws_geom": int(out[15]), "bind_descriptors": bool(out[16]),
                "paired_rows": int(out[17])}

    def run(self, X: torch.Tensor, Y: torch.Tensor, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        A, K = self.A, self.K
        ldx = _check_dense(X, self._x_rows, K, "X")
        ldy = _check_dense(Y, self.m_out, K, "Y")
        rp, ci, va = A.ptrs()
        call("smfv_plan_execute", self._plan, rp, ci, va, X.data_ptr(), ldx, Y.data_ptr(), ldy,
             stream_handle(stream))
        return Y

    @property
    def epilogue_mode(self) -> str | None:
        """None (no axpby), "fused" or "two_pass" (smfv_plan_epilogue_mode)."""
        mode = ctypes.c_int(0)
        call("smfv_plan_epilogue_mode", self._plan, byref(mode))
        return EPILOGUE_MODES[mode.value]

    def run_axpby(self, X: torch.Tensor, Y: torch.Tensor, alpha: float, beta: float,
                  stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Y = alpha * A * X + beta * Y in place (smfv_plan_execute_axpby); the
        plan must have been created with axpby.  beta == 0 does not read Y."""
        A, K = self.A, self.K
        ldx = _check_dense(X, self._x_rows, K, "X")
        ldy = _check_dense(Y, self.m_out, K, "Y")
        rp, ci, va = A.ptrs()
        call("smfv_plan_execute_axpby", self._plan, rp, ci, va, X.data_ptr(), ldx,
             ctypes.c_double(alpha), ctypes.c_double(beta), Y.data_ptr(), ldy, stream_handle(stream))
        return Y

    def __del__(self):
        try:
            if self._plan:
                call("smfv_plan_destroy", self._plan)
                self._plan = ctypes.c_void_p()
        except Exception:
            pass


def spmm(variant: int, A: DeviceCSR, X: torch.Tensor, Y: torch.Tensor | None = None,
         stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y = A * X on the device (asynchronous on `stream`), through A's cached
    plan for (variant, K)."""
    K = X.shape[1]
    if Y is None:
        Y = torch.empty((A.m, K), dtype=torch.float64, device=A.device)
    return A.plan(variant, K, stream).run(X, Y, stream)


def spmm_t(variant: int, A: DeviceCSR, X: torch.Tensor, Y: torch.Tensor | None = None,
           stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y = A^T * X on the device (X: A.m x K, Y: A.n x K; asynchronous on
    `stream`), through A's cached transposed plan for (variant, K)."""
    K = X.shape[1]
    if Y is None:
        Y = torch.empty((A.n, K), dtype=torch.float64, device=A.device)
    return A.plan(variant, K, stream, transpose=True).run(X, Y, stream)


TRSM_UPPER, TRSM_UNIT_DIAG, TRSM_NO_CHAIN, TRSM_CHAIN_ALL = 1, 2, 4, 8  # SMFV_TRSM_*
TRSM_STATS = 12  # SMFV_TRSM_STATS
TRSM_STAT_NAMES = ("levels", "widest_level", "launches", "chain_launches", "chain_rows", "chain_max_levels",
                   "strict_entries", "ignored_entries", "diag_entries", "plan_bytes", "analysis_ms", "thin_rows")


def trsm_flags(uplo: str = "lower", unit_diag: bool = False, chain: str = "auto", thin_rows: int = 0) -> int:
    """The SMFV_TRSM_* flags of a solve (ValueError for an unknown setting)."""
    if uplo not in ("lower", "upper"):
        raise ValueError(f"uplo must be 'lower' or 'upper', got {uplo!r}")
    if chain not in ("auto", "off", "all"):
        raise ValueError(f"chain must be 'auto', 'off' or 'all', got {chain!r}")
    if not 0 <= int(thin_rows) <= 0xffff:
        raise ValueError("thin_rows must be in [0, 65535]")
    return ((TRSM_UPPER if uplo == "upper" else 0) | (TRSM_UNIT_DIAG if unit_diag else 0)
            | {"auto": 0, "off": TRSM_NO_CHAIN, "all": TRSM_CHAIN_ALL}[chain] | (int(thin_rows) << 8))


def _trsm_stats(out) -> dict:
    return {k: (float(out[i]) if k == "analysis_ms" else int(out[i])) for i, k in enumerate(TRSM_STAT_NAMES)}


def trsm_analyse(A: SparseMatrix, K: int, uplo: str = "lower", unit_diag: bool = False, chain: str = "auto",
                 thin_rows: int = 0) -> dict:
    """The figures of a solve's host analysis (smfv_trsm_analyse; no device)."""
    ip = ctypes.POINTER(ctypes.c_int)
    rp = np.ascontiguousarray(A.rowPtr, dtype=np.int32)
    ci = np.ascontiguousarray(A.colIndices, dtype=np.int32)
    out = (ctypes.c_double * TRSM_STATS)()
    call("smfv_trsm_analyse", A.numRows, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), K,
         trsm_flags(uplo, unit_diag, chain, thin_rows), out)
    return _trsm_stats(out)


class TrsmPlan:
    """A triangular solve T Y = X analysed once for (pattern of A, K): T the
    lower (uplo="upper": the upper) triangle of the square A, the other
    triangle ignored, X and Y m x K (include/smfv.h, smfv_trsm_plan_*).  The
    result is bit-identical to sequential substitution in CSR order.
    unit_diag: the diagonal entries are ignored too and taken as 1.
    chain: "auto" runs each run of thin levels in one launch of a single block
    and each wide level as a grid launch; "off" / "all" force one launch per
    level / one launch in all (A/B, tests); thin_rows sets the threshold (A/B).
    The plan computes from its own copy of the values, written by
    bind_values(): bind again after A.values change."""

    def __init__(self, A: DeviceCSR, K: int, uplo: str = "lower", unit_diag: bool = False, chain: str = "auto",
                 stream: torch.cuda.Stream | None = None, thin_rows: int = 0):
        flags = trsm_flags(uplo, unit_diag, chain, thin_rows)
        if A.m != A.n:
            raise ValueError(f"a triangular solve needs a square matrix, got {A.m} x {A.n}")
        self.A, self.K, self.uplo, self.unit_diag, self.chain = A, int(K), uplo, bool(unit_diag), chain
        self._plan = ctypes.c_void_p()
        ip = ctypes.POINTER(ctypes.c_int)
        call("smfv_trsm_plan_create", byref(self._plan), A.m, A.nnz, A.h_row_ptr.ctypes.data_as(ip),
             A.h_col_idx.ctypes.data_as(ip), self.K, flags)
        self.bind_values(stream)

    def bind_values(self, stream: torch.cuda.Stream | None = None) -> None:
        """(Re)bind the plan to A's current device values: the values into plan order, and the pivots."""
        call("smfv_trsm_plan_bind_values", self._plan, self.A.values.data_ptr(), stream_handle(stream))
        self.bound_version = self.A.values_version()

    def stats(self) -> dict:
        out = (ctypes.c_double * TRSM_STATS)()
        call("smfv_trsm_plan_stats", self._plan, out)
        return _trsm_stats(out)

    def solve(self, X: torch.Tensor, Y: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Y = T^-1 X (asynchronous on `stream`); Y may be X itself (in place)."""
        A, K = self.A, self.K
        if Y is None:
            Y = torch.empty((A.m, K), dtype=torch.float64, device=A.device)
        ldx = _check_dense(X, A.m, K, "X")
        ldy = _check_dense(Y, A.m, K, "Y")
        call("smfv_trsm_plan_execute", self._plan, A.values.data_ptr(), X.data_ptr(), ldx, Y.data_ptr(), ldy,
             stream_handle(stream))
        return Y

    def __del__(self):
        try:
            if self._plan:
                call("smfv_trsm_plan_destroy", self._plan)
                self._plan = ctypes.c_void_p()
        except Exception:
            pass


def sptrsm(A: DeviceCSR, X: torch.Tensor, uplo: str = "lower", unit_diag: bool = False,
           Y: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y = T^-1 X on the device, T the lower / upper triangle of A, through
    A's cached solve plan for (K, uplo, unit_diag)."""
    return A.trsm_plan(X.shape[1], uplo, unit_diag, stream=stream).solve(X, Y, stream)


ILU0_NO_CHAIN, ILU0_CHAIN_ALL = 4, 8  # SMFV_ILU0_*
ILU0_STATS = 15  # SMFV_ILU0_STATS
ILU0_STAT_NAMES = ("levels", "widest_level", "launches", "chain_launches", "chain_rows", "chain_max_levels", "steps",
                   "pairs", "max_steps_per_row", "max_pairs_per_row", "long_rows", "lds_slot_entries", "plan_bytes",
                   "analysis_ms", "thin_rows")


def ilu0_flags(chain: str = "auto", thin_rows: int = 0) -> int:
    """The SMFV_ILU0_* flags of a factorisation (ValueError for an unknown setting)."""
    if chain not in ("auto", "off", "all"):
        raise ValueError(f"chain must be 'auto', 'off' or 'all', got {chain!r}")
    if not 0 <= int(thin_rows) <= 0xffff:
        raise ValueError("thin_rows must be in [0, 65535]")
    return {"auto": 0, "off": ILU0_NO_CHAIN, "all": ILU0_CHAIN_ALL}[chain] | (int(thin_rows) << 8)


def _ilu0_stats(out) -> dict:
    return {k: (float(out[i]) if k == "analysis_ms" else int(out[i])) for i, k in enumerate(ILU0_STAT_NAMES)}


def ilu0_analyse(A: SparseMatrix, chain: str = "auto", thin_rows: int = 0) -> dict:
    """The figures of a factorisation's host analysis (smfv_ilu0_analyse; no device)."""
    ip = ctypes.POINTER(ctypes.c_int)
    rp = np.ascontiguousarray(A.rowPtr, dtype=np.int32)
    ci = np.ascontiguousarray(A.colIndices, dtype=np.int32)
    out = (ctypes.c_double * ILU0_STATS)()
    call("smfv_ilu0_analyse", A.numRows, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), ilu0_flags(chain, thin_rows), out)
    return _ilu0_stats(out)


class Ilu0Plan:
    """The ILU(0) of the square A analysed once for its pattern
    (include/smfv.h, smfv_ilu0_plan_*): factor() gives the factors in A's CSR
    order -- strict-lower entries L (unit diagonal), the rest U --,
    bit-identical to the sequential loop of the header.  chain / thin_rows:
    as for TrsmPlan (A/B, tests).  The plan holds no values: factor() reads
    A.values as they are when it runs."""

    def __init__(self, A: DeviceCSR, chain: str = "auto", thin_rows: int = 0):
        flags = ilu0_flags(chain, thin_rows)
        if A.m != A.n:
            raise ValueError(f"ILU(0) needs a square matrix, got {A.m} x {A.n}")
        self.A, self.chain = A, chain
        self._plan = ctypes.c_void_p()
        ip = ctypes.POINTER(ctypes.c_int)
        call("smfv_ilu0_plan_create", byref(self._plan), A.m, A.nnz, A.h_row_ptr.ctypes.data_as(ip),
             A.h_col_idx.ctypes.data_as(ip), flags)

    def bind_values(self, stream: torch.cuda.Stream | None = None) -> None:
        """Nothing to do: the plan holds no values (DeviceCSR.values_changed()
        calls this on every cached plan)."""

    def stats(self) -> dict:
        out = (ctypes.c_double * ILU0_STATS)()
        call("smfv_ilu0_plan_stats", self._plan, out)
        return _ilu0_stats(out)

    def factor(self, out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The factors of A.values (asynchronous on `stream`) into `out`,
        which may be A.values itself (in place)."""
        A = self.A
        if out is None:
            out = torch.empty_like(A.values)
        if not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (A.nnz,) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 HIP tensor of {A.nnz} entries")
        call("smfv_ilu0_plan_factor", self._plan, A.values.data_ptr(), out.data_ptr(), stream_handle(stream))
        return out

    def __del__(self):
        try:
            if self._plan:
                call("smfv_ilu0_plan_destroy", self._plan)
                self._plan = ctypes.c_void_p()
        except Exception:
            pass


def ilu0(A: DeviceCSR, stream: torch.cuda.Stream | None = None) -> DeviceCSR:
    """The ILU(0) factors of A as a matrix of A's pattern, through A's cached plan."""
    return A.like(A.ilu0_plan().factor(stream=stream))


REORDER_TO_NEW, REORDER_TO_OLD, REORDER_STORE_NT = 1, 2, 4  # SMFV_REORDER_*
REORDER_STATS = 4  # SMFV_REORDER_STATS
REORDER_STAT_NAMES = ("m", "nnz", "plan_bytes", "create_ms")


class ReorderedCSR:
    """The square A under another numbering (include/smfv.h,
    smfv_reorder_plan_*): B = P A P^T with row i of B = row perm[i] of A and
    every row's entries in A's CSR order, so B (P X) == P (A X) bit for bit.
    order: "multicolor" (smfv_order_multicolor; `ncolors` and `color` are set,
    and B's triangles have at most `ncolors` levels) or a permutation array
    (`ncolors` is None).  B is a DeviceCSR with plans of its own; its values
    follow A.values: refresh() carries them over on the device, and `B`
    refreshes by itself when A.values_version() has moved.  to_new / to_old
    carry m x K blocks into B's numbering and back."""

    def __init__(self, A: DeviceCSR, order="multicolor"):
        if A.m != A.n:
            raise ValueError(f"a reordering needs a square matrix, got {A.m} x {A.n}")
        self.A = A
        if isinstance(order, str):
            if order != "multicolor":
                raise ValueError(f"order must be 'multicolor' or a permutation array, got {order!r}")
            self.perm, self.color, self.ncolors = multicolor_order_pattern(A.m, A.h_row_ptr, A.h_col_idx)
        else:
            self.perm, self.color, self.ncolors = np.ascontiguousarray(order, dtype=np.int32), None, None
        b_rp, b_ci, self.vperm = csr_permute_pattern(A.m, A.h_row_ptr, A.h_col_idx, self.perm)
        self._plan = ctypes.c_void_p()
        ip = ctypes.POINTER(ctypes.c_int)
        call("smfv_reorder_plan_create", byref(self._plan), A.m, A.nnz, self.perm.ctypes.data_as(ip),
             self.vperm.ctypes.data_as(ip))
        B = object.__new__(DeviceCSR)
        B.m, B.n, B.nnz = A.m, A.n, A.nnz
        B.h_row_ptr, B.h_col_idx = b_rp, b_ci
        B.row_ptr = torch.from_numpy(b_rp).to(A.device)
        B.col_idx = torch.from_numpy(b_ci).to(A.device)
        B.values = torch.empty_like(A.values)
        B.device = A.device
        B._plans = {}
        self._B = B
        self.refresh()

    @property
    def B(self) -> DeviceCSR:
        """The renumbered matrix, its values (and its cached plans) brought up
        to A.values first if those changed since the last refresh."""
        if self._version != self.A.values_version():
            self.refresh()
        return self._B

    def refresh(self, stream: torch.cuda.Stream | None = None) -> None:
        """B.values = A.values[vperm] on the device (asynchronous on `stream`),
        then B.values_changed(): the library writes B.values behind torch's
        version counter, so B's cached plans are bound again explicitly."""
        call("smfv_reorder_plan_values", self._plan, self.A.values.data_ptr(), self._B.values.data_ptr(),
             stream_handle(stream))
        self._version = self.A.values_version()
        self._B.values_changed(stream)

    def _rows(self, direction: int, X: torch.Tensor, out: torch.Tensor | None, stream, nt: bool) -> torch.Tensor:
        m = self.A.m
        if X.dim() != 2 or X.shape[1] < 1:
            raise ValueError(f"X must have shape ({m}, K) with K >= 1, got {tuple(X.shape)}")
        K = X.shape[1]
        if out is None:
            out = torch.empty((m, K), dtype=torch.float64, device=self.A.device)
        ldx = _check_dense(X, m, K, "X")
        ldy = _check_dense(out, m, K, "out")
        call("smfv_reorder_plan_rows", self._plan, direction | (REORDER_STORE_NT if nt else 0), X.data_ptr(), ldx, K,
             out.data_ptr(), ldy, stream_handle(stream))
        return out

    def to_new(self, X: torch.Tensor, out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
               nt: bool = False) -> torch.Tensor:
        """out[i] = X[perm[i]]: an m x K block into B's numbering (asynchronous
        on `stream`; out must not be X).  nt: non-temporal stores (A/B)."""
        return self._rows(REORDER_TO_NEW, X, out, stream, nt)

    def to_old(self, Y: torch.Tensor, out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
               nt: bool = False) -> torch.Tensor:
        """out[perm[i]] = Y[i]: back into A's numbering; undoes to_new."""
        return self._rows(REORDER_TO_OLD, Y, out, stream, nt)

    def stats(self) -> dict:
        out = (ctypes.c_double * REORDER_STATS)()
        call("smfv_reorder_plan_stats", self._plan, out)
        return {k: (float(out[i]) if k == "create_ms" else int(out[i])) for i, k in enumerate(REORDER_STAT_NAMES)}

    def __del__(self):
        try:
            if self._plan:
                call("smfv_reorder_plan_destroy", self._plan)
                self._plan = ctypes.c_void_p()
        except Exception:
            pass


class Ilu0Preconditioner:
    """M^-1 = U^-1 L^-1 for m x K blocks: owns F = A.like(...), A's Ilu0Plan
    and F's two solve plans (lower with a unit diagonal, upper).  refactor()
    after A.values changed; apply() runs the two solves.  chain goes to all
    three plans, thin_rows to the factorisation alone (the two kernels'
    thresholds are measured apart).
    reorder: None (natural order), "multicolor", a permutation array or a
    ReorderedCSR of A: the preconditioner then factors B = P A P^T and solves
    on B's factors, and apply() is to_new, the two solves, to_old, through a
    buffer allocated once (`R` is the ReorderedCSR).  A multicolour ILU(0) has
    as many levels as colours instead of the natural order's hundreds or
    thousands, and is a different, usually somewhat weaker, preconditioner."""

    def __init__(self, A: DeviceCSR, K: int, chain: str = "auto", stream: torch.cuda.Stream | None = None,
                 thin_rows: int = 0, reorder=None):
        self.A, self.K = A, int(K)
        self.R = None
        if reorder is not None:
            self.R = reorder if isinstance(reorder, ReorderedCSR) else ReorderedCSR(A, reorder)
            if self.R.A is not A:
                raise ValueError("reorder is a ReorderedCSR of another matrix")
            self.R.refresh(stream)
            self._w = torch.empty((A.m, self.K), dtype=torch.float64, device=A.device)
        M = self.M = A if self.R is None else self.R._B
        self.plan = Ilu0Plan(M, chain, thin_rows)
        self.F = M.like(torch.empty_like(M.values))
        self.plan.factor(self.F.values, stream)
        self.lower = TrsmPlan(self.F, self.K, "lower", True, chain, stream=stream)
        self.upper = TrsmPlan(self.F, self.K, "upper", False, chain, stream=stream)

    def refactor(self, stream: torch.cuda.Stream | None = None) -> None:
        """Factor A.values again and bind both solves to the new factors.  The
        library writes F.values behind torch's back (no version counter
        moves), so the solves are bound again explicitly.  With a reordering,
        B's values are refreshed from A's first."""
        if self.R is not None:
            self.R.refresh(stream)
        self.plan.factor(self.F.values, stream)
        self.lower.bind_values(stream)
        self.upper.bind_values(stream)

    def apply(self, X: torch.Tensor, Y: torch.Tensor | None = None,
              stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Y = U^-1 L^-1 X (asynchronous on `stream`); the intermediate
        L^-1 X lives in Y, which may be X itself.  With a reordering:
        Y = P^T U^-1 L^-1 P X with B's factors, the intermediates in the
        preconditioner's own buffer."""
        if self.R is None:
            Y = self.lower.solve(X, Y, stream)
            return self.upper.solve(Y, Y, stream)
        W = self.R.to_new(X, self._w, stream)
        self.lower.solve(W, W, stream)
        self.upper.solve(W, W, stream)
        return self.R.to_old(W, Y, stream)


COL_NEGATE, COL_ZERO_DEN = 1, 2  # SMFV_COL_*


def coldot_rule() -> tuple[int, int]:
    """(CHUNK, STRANDS) of the column-dot rule (smfv_coldot_rule)."""
    chunk, strands = ctypes.c_int(0), ctypes.c_int(0)
    call("smfv_coldot_rule", byref(chunk), byref(strands))
    return chunk.value, strands.value


def coldot_workspace_doubles(m: int, K: int) -> int:
    b = c_size_t(0)
    call("smfv_coldot_workspace_bytes", int(m), int(K), byref(b))
    return b.value // 8


def _block_shape(X: torch.Tensor, name: str) -> tuple[int, int]:
    if X.dim() != 2 or X.shape[1] < 1:
        raise ValueError(f"{name} must have shape (m, K) with K >= 1, got {tuple(X.shape)}")
    return int(X.shape[0]), int(X.shape[1])


def _check_cols(v: torch.Tensor | None, K: int, name: str, like: torch.Tensor) -> int:
    """A per-column array: K contiguous float64 entries on `like`'s device; its address (0 for None)."""
    if v is None:
        return 0
    if not v.is_cuda or v.dtype != torch.float64 or v.device != like.device:
        raise TypeError(f"{name} must be a float64 HIP tensor on {like.device}")
    if v.dim() != 1 or v.shape[0] != K or (K > 1 and v.stride(0) != 1):
        raise ValueError(f"{name} must be {K} contiguous entries, got shape {tuple(v.shape)}")
    return v.data_ptr()


def _same_device(X: torch.Tensor, Y: torch.Tensor, name: str) -> None:
    if Y.device != X.device:
        raise TypeError(f"{name} is on {Y.device}, not on {X.device}")


def coldot(X: torch.Tensor, Y: torch.Tensor, out: torch.Tensor | None = None,
           stream: torch.cuda.Stream | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """out[j] = sum_i X[i, j] * Y[i, j] in the fixed order of the column-dot
    rule (include/smfv.h; smfv_coldot_f64), asynchronous on `stream`.  X may
    be Y.  Without `out` / `workspace` (coldot_workspace_doubles entries) they
    are allocated here; a caller that captures passes both."""
    m, K = _block_shape(X, "X")
    ldx = _check_dense(X, m, K, "X")
    ldy = _check_dense(Y, m, K, "Y")
    _same_device(X, Y, "Y")
    if out is None:
        out = torch.empty(K, dtype=torch.float64, device=X.device)
    if workspace is None:
        workspace = torch.empty(coldot_workspace_doubles(m, K), dtype=torch.float64, device=X.device)
    elif not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous() \
            or workspace.numel() < coldot_workspace_doubles(m, K):
        raise ValueError(f"workspace must be a contiguous float64 HIP tensor of {coldot_workspace_doubles(m, K)} entries")
    call("smfv_coldot_f64", m, K, X.data_ptr(), ldx, Y.data_ptr(), ldy, _check_cols(out, K, "out", X),
         workspace.data_ptr(), stream_handle(stream))
    return out


def _col_flags(negate: bool, zero_den: bool) -> int:
    return (COL_NEGATE if negate else 0) | (COL_ZERO_DEN if zero_den else 0)


def _col_update(fn: str, num, den, X, Y, negate, zero_den, stream) -> torch.Tensor:
    m, K = _block_shape(X, "X")
    ldx = _check_dense(X, m, K, "X")
    ldy = _check_dense(Y, m, K, "Y")
    _same_device(X, Y, "Y")
    if num is None:
        raise TypeError("num must be a tensor of K entries")
    call(fn, m, K, _check_cols(num, K, "num", X), _check_cols(den, K, "den", X), _col_flags(negate, zero_den),
         X.data_ptr(), ldx, Y.data_ptr(), ldy, stream_handle(stream))
    return Y


def col_axpy(num: torch.Tensor, den: torch.Tensor | None, X: torch.Tensor, Y: torch.Tensor, negate: bool = False,
             zero_den: bool = False, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y[:, j] += s[j] * X[:, j] with s = num / den (den None: s = num) formed
    on the device (smfv_col_axpy_f64); negate flips s, zero_den makes s[j]
    +0.0 where den[j] == 0.  Y may be X."""
    return _col_update("smfv_col_axpy_f64", num, den, X, Y, negate, zero_den, stream)


def col_xpay(num: torch.Tensor, den: torch.Tensor | None, X: torch.Tensor, Y: torch.Tensor, negate: bool = False,
             zero_den: bool = False, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y[:, j] = X[:, j] + s[j] * Y[:, j] (smfv_col_xpay_f64); s as in col_axpy."""
    return _col_update("smfv_col_xpay_f64", num, den, X, Y, negate, zero_den, stream)


def pcg_update(num: torch.Tensor, den: torch.Tensor | None, P: torch.Tensor, Q: torch.Tensor, X: torch.Tensor,
               R: torch.Tensor, rr: torch.Tensor | None = None, negate: bool = False, zero_den: bool = False,
               stream: torch.cuda.Stream | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """X += s P, R -= s Q and rr = coldot(R, R) of the new R in one pass
    (smfv_pcg_update_f64), bit-identical to the three separate calls.  The
    four blocks must not overlap.  Returns rr."""
    m, K = _block_shape(X, "X")
    lds = [_check_dense(T, m, K, n) for T, n in ((P, "P"), (Q, "Q"), (X, "X"), (R, "R"))]
    for T, n in ((P, "P"), (Q, "Q"), (R, "R")):
        _same_device(X, T, n)
    if num is None:
        raise TypeError("num must be a tensor of K entries")
    if rr is None:
        rr = torch.empty(K, dtype=torch.float64, device=X.device)
    if workspace is None:
        workspace = torch.empty(coldot_workspace_doubles(m, K), dtype=torch.float64, device=X.device)
    elif not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous() \
            or workspace.numel() < coldot_workspace_doubles(m, K):
        raise ValueError(f"workspace must be a contiguous float64 HIP tensor of {coldot_workspace_doubles(m, K)} entries")
    call("smfv_pcg_update_f64", m, K, _check_cols(num, K, "num", X), _check_cols(den, K, "den", X),
         _col_flags(negate, zero_den), P.data_ptr(), lds[0], Q.data_ptr(), lds[1], X.data_ptr(), lds[2], R.data_ptr(),
         lds[3], _check_cols(rr, K, "rr", X), workspace.data_ptr(), stream_handle(stream))
    return rr


class BlockPCG:
    """Preconditioned conjugate gradients on K right-hand sides at once, every
    column a CG of its own (no Gram matrices): A X = B for a symmetric
    positive definite A.

    A: a DeviceCSR (a ROWWISE SpmmPlan is made) or a non-transposed SpmmPlan
    of the caller's.  M: anything with apply(X, Y, stream=...) computing
    Y = M^-1 X -- an Ilu0Preconditioner in either ordering --, or None for the
    identity: Z is R then, nothing is copied, and rz is rr (one dot fewer).
    Every block (X, R, P, Q, Z), the per-column scalars and the dot workspace
    are allocated here, once.

    An iteration is Q = A P; pq = coldot(P, Q); the fused update with
    s = rz / pq, which also gives rr; Z = M(R); rz' = coldot(R, Z);
    P = Z + (rz' / rz) P; rz <- rz'.  The quotients are formed on the device
    with the zero-denominator guard always on, so a column whose residual is
    exactly zero stays exactly where it is; converged columns keep iterating.
    iterate() makes no host read, allocation or synchronisation and captures
    into a graph.  rz and rz' swap buffers every iteration: capture an EVEN
    number of iterations, so that a replay starts where the capture did
    (solve(graph=True) keeps one graph per parity instead)."""

    def __init__(self, A, K: int, M=None, stream: torch.cuda.Stream | None = None):
        if isinstance(A, SpmmPlan):
            if A._transposed or A.rows is not None:
                raise ValueError("BlockPCG needs a plan of the whole A, not a transposed or a row-block plan")
            if A.K != int(K):
                raise ValueError(f"the plan was made for K = {A.K}, not {K}")
            self.plan, self.A = A, A.A
        elif isinstance(A, DeviceCSR):
            self.plan, self.A = SpmmPlan(Variant.ROWWISE, A, int(K), stream=stream), A
        else:
            raise TypeError("A must be a DeviceCSR or an SpmmPlan")
        if self.A.m != self.A.n:
            raise ValueError(f"BlockPCG needs a square matrix, got {self.A.m} x {self.A.n}")
        if M is not None and not callable(getattr(M, "apply", None)):
            raise TypeError("M must have apply(X, Y, stream=...) or be None")
        self.K, self.M, self.stream = int(K), M, stream
        m, dev = self.A.m, self.A.device
        new = lambda: torch.zeros((m, self.K), dtype=torch.float64, device=dev)  # noqa: E731
        self.X, self.R, self.P, self.Q = new(), new(), new(), new()
        self.Z = self.R if M is None else new()
        # rows: rz (even iterations), bb, rz (odd), pq, rr, bb again.  With M,
        # (rr, bb) are rows 4:6; without, rr is the current rz beside row 1.
        self._sc = torch.zeros((6, self.K), dtype=torch.float64, device=dev)
        self._one = torch.ones(self.K, dtype=torch.float64, device=dev)
        self._ws = torch.empty(coldot_workspace_doubles(m, self.K), dtype=torch.float64, device=dev)
        self._host = torch.empty((2, self.K), dtype=torch.float64).pin_memory()
        self._par = 0  # which of rows 0 / 2 holds rz
        self._graphs = None
        self.iterations = 0

    def _rz(self, par: int) -> torch.Tensor:
        return self._sc[2 * par]

    @property
    def rr(self) -> torch.Tensor:
        """R . R per column after the last iteration (on the device)."""
        return self._sc[4] if self.M is not None else self._rz(self._par)

    @property
    def bb(self) -> torch.Tensor:
        """B . B per column of the last start() (on the device)."""
        return self._sc[1]

    def start(self, B: torch.Tensor, X0: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> None:
        """R = B - A X0 (X0 None: X = 0, R = B, A is not launched), Z = M(R),
        P = Z, rz = coldot(R, Z), bb = coldot(B, B); asynchronous."""
        s = stream if stream is not None else self.stream
        m, K = self.A.m, self.K
        _check_dense(B, m, K, "B")
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
            self.R.copy_(B)
            if X0 is None:
                self.X.zero_()
            else:
                _check_dense(X0, m, K, "X0")
                self.X.copy_(X0)
                self.plan.run(self.X, self.Q, s)
                col_axpy(self._one, None, self.Q, self.R, negate=True, stream=s)  # R = B - A X0
            if self.M is not None:
                self.M.apply(self.R, self.Z, stream=s)
            self.P.copy_(self.Z)
            self._par = 0
            coldot(self.R, self.Z, self._rz(0), s, self._ws)
            coldot(B, B, self._sc[1], s, self._ws)
            self._sc[5].copy_(self._sc[1])
        self.iterations = 0

    def iterate(self, n: int = 1, stream: torch.cuda.Stream | None = None) -> None:
        """n iterations, launched back to back on `stream`: no host read, no
        allocation, no synchronisation."""
        s = stream if stream is not None else self.stream
        for _ in range(int(n)):
            rz, rz_new, pq = self._rz(self._par), self._rz(1 - self._par), self._sc[3]
            self.plan.run(self.P, self.Q, s)
            coldot(self.P, self.Q, pq, s, self._ws)
            if self.M is None:  # Z is R and rz' is rr
                pcg_update(rz, pq, self.P, self.Q, self.X, self.R, rz_new, zero_den=True, stream=s, workspace=self._ws)
            else:
                pcg_update(rz, pq, self.P, self.Q, self.X, self.R, self._sc[4], zero_den=True, stream=s,
                           workspace=self._ws)
                self.M.apply(self.R, self.Z, stream=s)
                coldot(self.R, self.Z, rz_new, s, self._ws)
            col_xpay(rz_new, rz, self.Z, self.P, zero_den=True, stream=s)
            self._par = 1 - self._par
        self.iterations += int(n)

    def residuals(self, stream: torch.cuda.Stream | None = None) -> tuple[np.ndarray, np.ndarray]:
        """(rr, bb) on the host: one read of 2 K doubles, then a wait for it."""
        s = stream if stream is not None else self.stream
        if self.M is not None:
            src, swap = self._sc[4:6], False
        else:  # rr is the current rz: rows (0, 1) or (1, 2)
            src, swap = (self._sc[0:2], False) if self._par == 0 else (self._sc[1:3], True)
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
            self._host.copy_(src, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        h = self._host.numpy().copy()
        return (h[1], h[0]) if swap else (h[0], h[1])

    def _capture(self, s) -> None:
        """One graph per parity of the rz buffers, each of one iteration."""
        side = s if s is not None else torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        par, its = self._par, self.iterations
        self._graphs = {}
        for p in (par, 1 - par):
            g = torch.cuda.CUDAGraph()
            assert self._par == p
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    self.iterate(1, side)
            self._graphs[p] = g
        self._par, self.iterations = par, its  # a capture executes nothing
        torch.cuda.current_stream().wait_stream(side)

    def solve(self, B: torch.Tensor, X0: torch.Tensor | None = None, tol: float = 1e-8, max_iters: int = 1000,
              check_every: int = 1, graph: bool = False):
        """Iterates until every column has rr[j] <= (tol * tol) * bb[j]
        (evaluated in fp64 on the host from one read of 2 K doubles every
        `check_every` iterations) or max_iters is reached.  graph: replay
        captured iterations instead of launching them.  Returns (X, the
        iteration count, rr / bb per column as a numpy array; 0 for a zero
        right-hand side met exactly)."""
        if check_every < 1 or max_iters < 0:
            raise ValueError("check_every must be at least 1 and max_iters non-negative")
        s = self.stream
        self.start(B, X0, s)
        if graph and self._graphs is None:
            self._capture(s)
        rr = bb = None
        while self.iterations < max_iters:
            n = min(int(check_every), max_iters - self.iterations)
            if graph:
                with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
                    for _ in range(n):
                        self._graphs[self._par].replay()
                        self._par = 1 - self._par
                self.iterations += n
            else:
                self.iterate(n, s)
            rr, bb = self.residuals(s)
            if bool(np.all(rr <= (tol * tol) * bb)):
                break
        if rr is None:
            rel = np.full(self.K, np.nan)
        else:
            with np.errstate(all="ignore"):
                rel = np.where(bb == 0.0, np.where(rr == 0.0, 0.0, np.inf), rr / bb)
        return self.X, self.iterations, rel


BLOCK_NEGATE = 1  # SMFV_BLOCK_NEGATE
BLOCK_MAX_K = 128  # SMFV_BLOCK_MAX_K


def gram_workspace_doubles(m: int, Kx: int, Ky: int) -> int:
    b = c_size_t(0)
    call("smfv_gram_workspace_bytes", int(m), int(Kx), int(Ky), byref(b))
    return b.value // 8


def gram_set_tiling(tiling: int = 0) -> None:
    """Force a register tiling of k_gram_partial (tests, A/B runs): 0 = by
    (Kx, Ky), 1 = 4 x 8, 2 = 2 x 4, 3 = 1 x 1.  The bits do not depend on it."""
    call("smfv_gram_set_tiling", int(tiling))


def _check_small(T: torch.Tensor, rows: int, cols: int, name: str, like: torch.Tensor) -> int:
    """A small dense matrix on `like`'s device: (rows, cols), row-major; its leading dimension."""
    if not T.is_cuda or T.dtype != torch.float64 or T.device != like.device:
        raise TypeError(f"{name} must be a float64 HIP tensor on {like.device}")
    if T.dim() != 2 or tuple(T.shape) != (rows, cols):
        raise ValueError(f"{name} must have shape ({rows}, {cols}), got {tuple(T.shape)}")
    if cols > 1 and T.stride(1) != 1:
        raise ValueError(f"{name} must be row-major (unit column stride)")
    return max(int(T.stride(0)), cols) if rows > 1 else cols


def gram(X: torch.Tensor, Y: torch.Tensor, out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None,
         workspace: torch.Tensor | None = None) -> torch.Tensor:
    """out = X^T Y (Kx x Ky), every entry in the fixed order of the column-dot
    rule: out[i, j] == coldot(X[:, i], Y[:, j]) bit for bit (smfv_gram_f64),
    asynchronous on `stream`.  X may be Y; Kx and Ky are at most 128.  Without
    `out` / `workspace` (gram_workspace_doubles entries) they are allocated
    here; a caller that captures passes both."""
    m, Kx = _block_shape(X, "X")
    my, Ky = _block_shape(Y, "Y")
    if my != m:
        raise ValueError(f"X has {m} rows, Y has {my}")
    ldx = _check_dense(X, m, Kx, "X")
    ldy = _check_dense(Y, m, Ky, "Y")
    _same_device(X, Y, "Y")
    if out is None:
        out = torch.empty((Kx, Ky), dtype=torch.float64, device=X.device)
    ldg = _check_small(out, Kx, Ky, "out", X)
    need = gram_workspace_doubles(m, Kx, Ky)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=X.device)
    elif not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous() \
            or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous float64 HIP tensor of {need} entries")
    call("smfv_gram_f64", m, Kx, Ky, X.data_ptr(), ldx, Y.data_ptr(), ldy, out.data_ptr(), ldg, workspace.data_ptr(),
         stream_handle(stream))
    return out


def block_mul(X: torch.Tensor, C: torch.Tensor, Z: torch.Tensor | None = None, Y: torch.Tensor | None = None,
              negate: bool = False, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Y = Z + X C (Z None: Y = X C), or Y = Z - X C with negate; per entry
    the products are added to Z[i, j] one by one for l ascending
    (smfv_block_mul_f64).  X is m x Kx, C is Kx x Ky on the device, Z and Y
    are m x Ky.  Y may be Z, and Y may be X when Kx == Ky; any other overlap
    is refused.  Without Y a new block is returned."""
    m, Kx = _block_shape(X, "X")
    if C.dim() != 2 or C.shape[0] != Kx:
        raise ValueError(f"C must have shape ({Kx}, Ky), got {tuple(C.shape)}")
    Ky = int(C.shape[1])
    ldx = _check_dense(X, m, Kx, "X")
    ldc = _check_small(C, Kx, Ky, "C", X)
    if Y is None:
        Y = torch.empty((m, Ky), dtype=torch.float64, device=X.device)
    ldy = _check_dense(Y, m, Ky, "Y")
    _same_device(X, Y, "Y")
    ldz = 0
    if Z is not None:
        ldz = _check_dense(Z, m, Ky, "Z")
        _same_device(X, Z, "Z")
    call("smfv_block_mul_f64", m, Kx, Ky, BLOCK_NEGATE if negate else 0, X.data_ptr(), ldx, C.data_ptr(), ldc,
         Z.data_ptr() if Z is not None else 0, ldz, Y.data_ptr(), ldy, stream_handle(stream))
    return Y


def small_solve(G: torch.Tensor, H: torch.Tensor, out: torch.Tensor | None = None,
                stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """out = G^-1 H for a K x K matrix G and a K x N matrix H on the device
    (K, N <= 128): LU without pivoting and two substitutions in one launch
    (smfv_small_solve_f64), no host read.  A zero pivot gives what IEEE gives.
    `out` may be H."""
    if G.dim() != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1:
        raise ValueError(f"G must be square, got {tuple(G.shape)}")
    if not G.is_cuda or G.dtype != torch.float64:
        raise TypeError("G must be a float64 HIP tensor")
    K = int(G.shape[0])
    if H.dim() != 2 or H.shape[0] != K or H.shape[1] < 1:
        raise ValueError(f"H must have shape ({K}, N), got {tuple(H.shape)}")
    N = int(H.shape[1])
    ldg = _check_small(G, K, K, "G", G)
    ldh = _check_small(H, K, N, "H", G)
    if out is None:
        out = torch.empty((K, N), dtype=torch.float64, device=G.device)
    ldc = _check_small(out, K, N, "out", G)
    call("smfv_small_solve_f64", K, N, G.data_ptr(), ldg, H.data_ptr(), ldh, out.data_ptr(), ldc, stream_handle(stream))
    return out


class CoupledBlockPCG:
    """Block preconditioned conjugate gradients (O'Leary) on K right-hand
    sides: A X = B for a symmetric positive definite A, the columns coupled
    through K x K Gram matrices.  Every step searches the whole K-dimensional
    block space, so it needs fewer iterations than BlockPCG, whose columns are
    K conjugate-gradient runs of their own.

    A, M, K and the methods are BlockPCG's: A a DeviceCSR (a ROWWISE SpmmPlan
    is made) or a non-transposed SpmmPlan, M anything with
    apply(X, Y, stream=...) or None; K is at most 128.  Every block (X, R, P,
    Q, Z), the K x K matrices and the Gram workspace are allocated here, once.

    start: R = B - A X0, Z = M(R), P = Z, rho = gram(Z, R), bb = coldot(B, B).
    An iteration is Q = A P; Gamma = gram(P, Q); alpha = small_solve(Gamma,
    rho); X += P alpha; R -= Q alpha; Z = M(R); rho' = gram(Z, R);
    beta = small_solve(rho, rho'); P = Z + P beta; rho <- rho' by swapping
    buffers.  rr is diag(rho') when M is None, else one coldot(R, R).
    iterate() makes no host read, allocation or synchronisation and captures
    into a graph; as in BlockPCG the rho buffers swap every iteration, so
    capture an EVEN number of iterations (solve(graph=True) keeps one graph
    per parity).

    Limits.  There is no breakdown guard like BlockPCG's zero-denominator
    flag: a rank-deficient block -- a zero or repeated right-hand-side column,
    or columns that become dependent as they converge -- makes Gamma or rho
    singular, and the IEEE infinities and NaNs propagate into every column.
    solve() stops at the first check where any rr is non-finite, sets
    self.breakdown = True and returns as usual.  Deflation and the
    QR-stabilised variants are out of scope."""

    def __init__(self, A, K: int, M=None, stream: torch.cuda.Stream | None = None):
        if isinstance(A, SpmmPlan):
            if A._transposed or A.rows is not None:
                raise ValueError("CoupledBlockPCG needs a plan of the whole A, not a transposed or a row-block plan")
            if A.K != int(K):
                raise ValueError(f"the plan was made for K = {A.K}, not {K}")
            self.plan, self.A = A, A.A
        elif isinstance(A, DeviceCSR):
            if not 1 <= int(K) <= BLOCK_MAX_K:
                raise ValueError(f"K = {K}, must be in 1..{BLOCK_MAX_K}")
            self.plan, self.A = SpmmPlan(Variant.ROWWISE, A, int(K), stream=stream), A
        else:
            raise TypeError("A must be a DeviceCSR or an SpmmPlan")
        if not 1 <= int(K) <= BLOCK_MAX_K:
            raise ValueError(f"K = {K}, must be in 1..{BLOCK_MAX_K}")
        if self.A.m != self.A.n:
            raise ValueError(f"CoupledBlockPCG needs a square matrix, got {self.A.m} x {self.A.n}")
        if M is not None and not callable(getattr(M, "apply", None)):
            raise TypeError("M must have apply(X, Y, stream=...) or be None")
        self.K, self.M, self.stream = int(K), M, stream
        m, dev = self.A.m, self.A.device
        new = lambda: torch.zeros((m, self.K), dtype=torch.float64, device=dev)  # noqa: E731
        self.X, self.R, self.P, self.Q = new(), new(), new(), new()
        self.Z = self.R if M is None else new()
        # K x K: rho (even iterations), rho (odd), Gamma, alpha, beta
        self._sm = torch.zeros((5, self.K, self.K), dtype=torch.float64, device=dev)
        self._rrbb = torch.zeros((2, self.K), dtype=torch.float64, device=dev)  # rr (with M, or gathered), bb
        self._one = torch.ones(self.K, dtype=torch.float64, device=dev)
        self._ws = torch.empty(gram_workspace_doubles(m, self.K, self.K), dtype=torch.float64, device=dev)
        self._host = torch.empty((2, self.K), dtype=torch.float64).pin_memory()
        self._par = 0  # which of the two rho buffers holds rho
        self._graphs = None
        self.iterations = 0
        self.breakdown = False

    def _rho(self, par: int) -> torch.Tensor:
        return self._sm[par]

    @property
    def rr(self) -> torch.Tensor:
        """R . R per column after the last iteration (on the device)."""
        return self._rrbb[0] if self.M is not None else self._rho(self._par).diagonal()

    @property
    def bb(self) -> torch.Tensor:
        """B . B per column of the last start() (on the device)."""
        return self._rrbb[1]

    def start(self, B: torch.Tensor, X0: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> None:
        """R = B - A X0 (X0 None: X = 0, R = B, A is not launched), Z = M(R),
        P = Z, rho = gram(Z, R), bb = coldot(B, B); asynchronous."""
        s = stream if stream is not None else self.stream
        m, K = self.A.m, self.K
        _check_dense(B, m, K, "B")
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
            self.R.copy_(B)
            if X0 is None:
                self.X.zero_()
            else:
                _check_dense(X0, m, K, "X0")
                self.X.copy_(X0)
                self.plan.run(self.X, self.Q, s)
                col_axpy(self._one, None, self.Q, self.R, negate=True, stream=s)  # R = B - A X0
            if self.M is not None:
                self.M.apply(self.R, self.Z, stream=s)
            self.P.copy_(self.Z)
            self._par = 0
            gram(self.Z, self.R, self._rho(0), s, self._ws)
            coldot(B, B, self._rrbb[1], s, self._ws)
        self.iterations = 0
        self.breakdown = False

    def iterate(self, n: int = 1, stream: torch.cuda.Stream | None = None) -> None:
        """n iterations, launched back to back on `stream`: no host read, no
        allocation, no synchronisation."""
        s = stream if stream is not None else self.stream
        gamma, alpha, beta = self._sm[2], self._sm[3], self._sm[4]
        for _ in range(int(n)):
            rho, rho_new = self._rho(self._par), self._rho(1 - self._par)
            self.plan.run(self.P, self.Q, s)
            gram(self.P, self.Q, gamma, s, self._ws)
            small_solve(gamma, rho, alpha, s)
            block_mul(self.P, alpha, self.X, self.X, stream=s)
            block_mul(self.Q, alpha, self.R, self.R, negate=True, stream=s)
            if self.M is not None:
                self.M.apply(self.R, self.Z, stream=s)
            gram(self.Z, self.R, rho_new, s, self._ws)
            if self.M is not None:
                coldot(self.R, self.R, self._rrbb[0], s, self._ws)
            small_solve(rho, rho_new, beta, s)
            block_mul(self.P, beta, self.Z, self.P, stream=s)
            self._par = 1 - self._par
        self.iterations += int(n)

    def residuals(self, stream: torch.cuda.Stream | None = None) -> tuple[np.ndarray, np.ndarray]:
        """(rr, bb) on the host: one read of 2 K doubles, then a wait for it."""
        s = stream if stream is not None else self.stream
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
            if self.M is None:  # rr is the diagonal of the current rho: gathered beside bb
                self._rrbb[0].copy_(self._rho(self._par).diagonal())
            self._host.copy_(self._rrbb, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        h = self._host.numpy().copy()
        return h[0], h[1]

    def _capture(self, s) -> None:
        """One graph per parity of the rho buffers, each of one iteration."""
        side = s if s is not None else torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        par, its = self._par, self.iterations
        self._graphs = {}
        for p in (par, 1 - par):
            g = torch.cuda.CUDAGraph()
            assert self._par == p
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    self.iterate(1, side)
            self._graphs[p] = g
        self._par, self.iterations = par, its  # a capture executes nothing
        torch.cuda.current_stream().wait_stream(side)

    def solve(self, B: torch.Tensor, X0: torch.Tensor | None = None, tol: float = 1e-8, max_iters: int = 1000,
              check_every: int = 1, graph: bool = False):
        """Iterates until every column has rr[j] <= (tol * tol) * bb[j]
        (evaluated in fp64 on the host from one read of 2 K doubles every
        `check_every` iterations), max_iters is reached, or some rr is
        non-finite (self.breakdown = True).  graph: replay captured
        iterations instead of launching them.  Returns (X, the iteration
        count, rr / bb per column as a numpy array; 0 for a zero right-hand
        side met exactly)."""
        if check_every < 1 or max_iters < 0:
            raise ValueError("check_every must be at least 1 and max_iters non-negative")
        s = self.stream
        self.start(B, X0, s)
        if graph and self._graphs is None:
            self._capture(s)
        rr = bb = None
        while self.iterations < max_iters:
            n = min(int(check_every), max_iters - self.iterations)
            if graph:
                with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
                    for _ in range(n):
                        self._graphs[self._par].replay()
                        self._par = 1 - self._par
                self.iterations += n
            else:
                self.iterate(n, s)
            rr, bb = self.residuals(s)
            if not bool(np.all(np.isfinite(rr))):
                self.breakdown = True
                break
            if bool(np.all(rr <= (tol * tol) * bb)):
                break
        if rr is None:
            rel = np.full(self.K, np.nan)
        else:
            with np.errstate(all="ignore"):
                rel = np.where(bb == 0.0, np.where(rr == 0.0, 0.0, np.inf), rr / bb)
        return self.X, self.iterations, rel


def spmm_rowblock(A: DeviceCSR, row_begin: int, row_end: int, X: torch.Tensor, Yblock: torch.Tensor,
                  stream=None) -> torch.Tensor:
    K = X.shape[1]
    ldx = _check_dense(X, A.n, K, "X")
    ldy = _check_dense(Yblock, row_end - row_begin, K, "Yblock")
    rp, ci, va = A.ptrs()
    call("smfv_spmm_rowblock_f64", row_begin, row_end, A.n, rp, ci, va, X.data_ptr(), ldx, K,
         Yblock.data_ptr(), ldy, stream_handle(stream))
    return Yblock


def spmm_colpanel(A: DeviceCSR, col_begin: int, col_end: int, X: torch.Tensor, panel: torch.Tensor,
                  stream=None) -> torch.Tensor:
    K = X.shape[1]
    ldx = _check_dense(X, A.n, K, "X")
    ldp = _check_dense(panel, A.m, col_end - col_begin, "panel")
    rp, ci, va = A.ptrs()
    call("smfv_spmm_colpanel_f64", A.m, A.n, col_begin, col_end, rp, ci, va, X.data_ptr(), ldx,
         panel.data_ptr(), max(ldp, 1), stream_handle(stream))
    return panel


def nnz_range_rows(A_host_row_ptr: np.ndarray, nnz_begin: int, nnz_end: int) -> tuple[int, int]:
    rp = np.ascontiguousarray(A_host_row_ptr, dtype=np.int32)
    rf, rl = ctypes.c_int(0), ctypes.c_int(0)
    call("smfv_nnz_range_rows", len(rp) - 1, rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
         nnz_begin, nnz_end, byref(rf), byref(rl))
    return rf.value, rl.value


def spmm_nnzrange(A: DeviceCSR, nnz_begin: int, nnz_end: int, X: torch.Tensor, stream=None):
    """Partial rows of the nnz range (SC/...NonZeroElement.cpp:56-67):
    returns (row_first, row_last, Ypart[(row_last-row_first+1) x K])."""
    K = X.shape[1]
    ldx = _check_dense(X, A.n, K, "X")
    rf, rl = nnz_range_rows(A.h_row_ptr, nnz_begin, nnz_end)
    nr = max(0, rl - rf + 1)
    Yp = torch.empty((nr, K), dtype=torch.float64, device=A.device)
    b = c_size_t(0)
    call("smfv_spmm_nnzrange_workspace_bytes", nr, nnz_end - nnz_begin, K, byref(b))
    ws = torch.empty(max(b.value, 1), dtype=torch.uint8, device=A.device)
    rp, ci, va = A.ptrs()
    call("smfv_spmm_nnzrange_f64", rf, rl, nnz_begin, nnz_end, A.n, rp, ci, va, X.data_ptr(), ldx, K,
         Yp.data_ptr(), max(K, 1), ws.data_ptr(), b.value, stream_handle(stream))
    return rf, rl, Yp


def compare(A: torch.Tensor, B: torch.Tensor, stream=None) -> tuple[float, float]:
    """Device areMatricesEqual (SC/utils.cpp:38-63): (max abs diff, max rel diff)."""
    m, K = A.shape
    lda = _check_dense(A, m, K, "A")
    ldb = _check_dense(B, m, K, "B")
    out = (ctypes.c_double * 2)()
    call("smfv_compare_f64", m, K, A.data_ptr(), lda, B.data_ptr(), ldb, out, stream_handle(stream))
    return out[0], out[1]


def fill_x_hash(X: torch.Tensor, seed: int, stream=None) -> torch.Tensor:
    n, K = X.shape
    ldx = _check_dense(X, n, K, "X")
    call("smfv_fill_x_hash_f64", n, K, seed, X.data_ptr(), ldx, stream_handle(stream))
    return X


# ---------------------------------------------------------------------------
# the reference's four functions (host arrays in, host array out)
# ---------------------------------------------------------------------------
def _run_host(variant: Variant, A: SparseMatrix, fatVector, vecCols: int) -> np.ndarray:
    X = np.ascontiguousarray(np.asarray(fatVector, dtype=np.float64).reshape(A.numCols, vecCols))
    dA = DeviceCSR(A)
    dX = torch.from_numpy(X).to(dA.device)
    Y = spmm(variant, dA, dX)
    return Y.cpu().numpy()


def sparseMatrixFatVectorMultiply(sparseMatrix: SparseMatrix, fatVector, vecCols: int) -> np.ndarray:
    return _run_host(Variant.SEQUENTIAL, sparseMatrix, fatVector, vecCols)


def _collective(variant: Variant, A: SparseMatrix, fatVector, vecCols: int, comm) -> np.ndarray:
    if comm is None or comm.size == 1:
        return _run_host(variant, A, fatVector, vecCols)
    from .dist import dist_spmm
    dA = DeviceCSR(A)
    X = np.ascontiguousarray(np.asarray(fatVector, dtype=np.float64).reshape(A.numCols, vecCols))
    dX = torch.from_numpy(X).to(dA.device)
    Y = dist_spmm(comm, variant, dA, dX, to_all=False, root=0)
    torch.cuda.synchronize()
    return Y.cpu().numpy() if comm.rank == 0 else np.empty((0, vecCols))


def sparseMatrixFatVectorMultiplyRowWise(sparseMatrix: SparseMatrix, fatVector, vecCols: int,
                                         comm=None) -> np.ndarray:
    return _collective(Variant.ROWWISE, sparseMatrix, fatVector, vecCols, comm)


def sparseMatrixFatVectorMultiplyColumnWise(sparseMatrix: SparseMatrix, fatVector, vecCols: int,
                                            comm=None) -> np.ndarray:
    return _collective(Variant.COLUMNWISE, sparseMatrix, fatVector, vecCols, comm)


def sparseMatrixFatVectorMultiplyNonZeroElement(sparseMatrix: SparseMatrix, fatVector, vecCols: int,
                                                comm=None) -> np.ndarray:
    return _collective(Variant.NONZERO, sparseMatrix, fatVector, vecCols, comm)


class VendorSpmm:
    """rocSPARSE generic SpMM on the same device operands (smfv_vendor_spmm_*):
    the vendor-library comparator, the analogue of the reference's PETSc
    MatMatMult block (SC/main.cpp:289-402).  Not the product path.
    alg: 0 rocSPARSE default, 1 CSR row split, 2 CSR merge path."""

    def __init__(self, A: DeviceCSR, X: torch.Tensor, Y: torch.Tensor, alg: int = 0,
                 stream: torch.cuda.Stream | None = None):
        K = X.shape[1]
        ldx = _check_dense(X, A.n, K, "X")
        ldy = _check_dense(Y, A.m, K, "Y")
        self.A, self.X, self.Y = A, X, Y  # keep the bound operands alive
        self._h = ctypes.c_void_p()
        rp, ci, va = A.ptrs()
        call("smfv_vendor_spmm_create", byref(self._h), alg, A.m, A.n, A.nnz, rp, ci, va, X.data_ptr(), ldx, K,
             Y.data_ptr(), ldy, stream_handle(stream))

    def run(self) -> torch.Tensor:
        call("smfv_vendor_spmm_execute", self._h)
        return self.Y

    def __del__(self):
        try:
            if self._h:
                call("smfv_vendor_spmm_destroy", self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass
