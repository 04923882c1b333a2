"""MI355X-native CSR x fat-vector SpMM engine (drop-in for the hot path of
AlexisBalayre/SparseMatrixMultiplicationMPI).

    Y[m x K] = A_csr[m x n] * X[n x K]   (fp64)
    Y[n x K] = A_csr^T * X[m x K]        (transposed plans, spmm_t)
    T Y = X, T a triangle of A_csr       (level-scheduled solves, sptrsm)
    L U ~ A_csr on A's pattern           (ILU(0), ilu0 / Ilu0Preconditioner)
    B = P A P^T, few levels              (multicolour reordering, DeviceCSR.reordered)
    d[j] = X[:, j] . Y[:, j], Y += s X   (fixed-order column dots, scaled updates, BlockPCG)
    G = X^T Y, Y = Z +- X C, C = G^-1 H  (Gram matrices, block updates, small solves, CoupledBlockPCG)

The product is libsmfv.so (HIP kernels for gfx950 + C ABI in include/smfv.h)
and libsmfv_mpi.so / smfv_main (the reference's C++ call surface and CLI).
This package is the Python host binding used by the tests and bench.py.
"""
from ._lib import LIB_PATH, SmfvError, lib  # noqa: F401  (raises if the library is missing)
from .inputs import (  # noqa: F401
    COP20K_M,
    COP20K_NNZ,
    SparseMatrix,
    areMatricesEqual,
    cop20k_surrogate,
    csr_permute,
    csr_transpose,
    deserialize,
    gen_fem27,
    gen_random_rows,
    generateLargeFatVector,
    multicolor_order,
    readMatrixMarketFile,
    serialize,
    writeMatrixMarketFile,
)
from .engine import (  # noqa: F401
    BLOCK_NEGATE,
    BlockPCG,
    CoupledBlockPCG,
    DeviceCSR,
    Ilu0Plan,
    Ilu0Preconditioner,
    ReorderedCSR,
    SpmmPlan,
    TrsmPlan,
    VendorSpmm,
    Variant,
    block_mul,
    col_axpy,
    col_xpay,
    coldot,
    coldot_rule,
    compare,
    ilu0,
    ilu0_analyse,
    fill_x_hash,
    gram,
    gram_workspace_doubles,
    pcg_update,
    small_solve,
    sparseMatrixFatVectorMultiply,
    sparseMatrixFatVectorMultiplyColumnWise,
    sparseMatrixFatVectorMultiplyNonZeroElement,
    sparseMatrixFatVectorMultiplyRowWise,
    spmm,
    spmm_t,
    sptrsm,
    trsm_analyse,
)

__version__ = "0.1.0"
