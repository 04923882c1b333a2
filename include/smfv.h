/*
 * smfv.h -- C ABI of the MI355X-native CSR x fat-vector SpMM engine.
 *
 *   Y[m x K] = A_csr[m x n] * X[n x K]        (fp64, int32 CSR indices)
 *
 * This is the drop-in boundary for the reference's hot path
 * (AlexisBalayre/SparseMatrixMultiplicationMPI, "Source Code/" = SC/):
 *
 *   reference interface (replaced)                              entry point here
 *   ---------------------------------------------------------  ---------------------------
 *   SC/SparseMatrixFatVectorMultiply.h:14-15  (sequential)      smfv_spmm_csr_f64(SMFV_SEQUENTIAL)
 *   SC/SparseMatrixFatVectorMultiplyRowWise.h:15-17             smfv_spmm_csr_f64(SMFV_ROWWISE),
 *                                                               smfv_dist_spmm_f64(SMFV_ROWWISE)
 *   SC/SparseMatrixFatVectorMultiplyColumnWise.h:15             smfv_spmm_csr_f64(SMFV_COLUMNWISE),
 *                                                               smfv_dist_spmm_f64(SMFV_COLUMNWISE)
 *   SC/SparseMatrixFatVectorMultiplyNonZeroElement.h:15         smfv_spmm_csr_f64(SMFV_NONZERO),
 *                                                               smfv_dist_spmm_f64(SMFV_NONZERO)
 *   SC/MatrixDefinitions.h:14-22 (SparseMatrix, FatVector)      plain pointers + sizes below
 *   partition formulas SC/...RowWise.cpp:26-29,                 smfv_partition_{rows,cols,nnz}
 *     ...ColumnWise.cpp:25-28, ...NonZeroElement.cpp:24-39
 *   SC/utils.cpp:38-63 (areMatricesEqual)                       smfv_compare_f64 (device-side)
 *
 * The C++ signatures of the reference (FatVector by value, MPI collective)
 * are kept verbatim in include/SparseMatrixFatVectorMultiply*.h; they are
 * thin host wrappers over this ABI (libsmfv_mpi.so).
 *
 * Conventions (all functions):
 *   - every pointer named d_* is a DEVICE pointer on the current HIP device;
 *   - CSR is 0-based: row_ptr[m+1], col_idx[nnz], values[nnz], with
 *     row_ptr[0] == 0 and row_ptr[m] == nnz (as built by SC/utils.cpp:162-181);
 *   - X and Y are row-major with leading dimensions ldx >= K, ldy >= K
 *     (the SC/utils.cpp:216-228 `serialize` layout when ld == K);
 *   - `stream` is a hipStream_t (NULL = default stream); every call is
 *     asynchronous on it and captures into a hipGraph (no allocation, no
 *     synchronisation inside);
 *   - results of SEQUENTIAL, ROWWISE and COLUMNWISE are bit-identical to the
 *     reference's sequential kernel (per-row nnz-ascending sums, separate
 *     multiply and add); NONZERO (merge-path) sums a row split across
 *     partitions in a different association, like the reference's own
 *     MPI_Reduce(SUM) -- deterministic, within 1e-12 relative in practice;
 *   - return value: SMFV_OK (0) or a negative smfv_status; the message of
 *     the last failure on the calling thread is smfv_last_error().  No C++
 *     exception crosses this boundary.
 */
#ifndef SMFV_H
#define SMFV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMFV_API __attribute__((visibility("default")))

typedef enum smfv_variant {
    SMFV_SEQUENTIAL = 0, /* SC/SparseMatrixFatVectorMultiply.cpp:11-31            */
    SMFV_ROWWISE = 1,    /* SC/SparseMatrixFatVectorMultiplyRowWise.cpp:12-126    */
    SMFV_COLUMNWISE = 2, /* SC/SparseMatrixFatVectorMultiplyColumnWise.cpp:13-131 */
    SMFV_NONZERO = 3     /* SC/SparseMatrixFatVectorMultiplyNonZeroElement.cpp:12-120 */
} smfv_variant;

typedef enum smfv_status {
    SMFV_OK = 0,
    SMFV_ERR_INVALID = -1,   /* bad sizes / null pointers / unknown variant */
    SMFV_ERR_WORKSPACE = -2, /* workspace missing or too small            */
    SMFV_ERR_HIP = -3,       /* a HIP runtime call failed                 */
    SMFV_ERR_COMM = -4,      /* an RCCL call failed                       */
    SMFV_ERR_HOST = -5       /* host-side failure (I/O, allocation)       */
} smfv_status;

/* ---- library ------------------------------------------------------------ */
SMFV_API const char *smfv_last_error(void);
SMFV_API const char *smfv_version(void);
/* Creates the HIP context on the current device, loads the library's code
 * object (one empty kernel launch on `stream`) and starts the runtime's
 * host<->device copy path (one 1 MiB copy each way: the process's first
 * copy of that size costs 10-30 ms once), synchronised: the one-time device
 * start-up a CPU caller never pays, done before a timed call so that call's
 * time is the SpMM's. */
SMFV_API int smfv_device_init(void *stream);

/* ---- partitions (pure host functions, no device needed) ----------------- */
/* RowWise: q = m/p, rows [r*q + min(r, m%p), +q + (r < m%p))  (RowWise.cpp:26-29) */
SMFV_API void smfv_partition_rows(int m, int p, int r, int *start, int *end);
/* ColumnWise: K/p columns, remainder to the LAST rank        (ColumnWise.cpp:25-28) */
SMFV_API void smfv_partition_cols(int K, int p, int r, int *start, int *end);
/* NonZeroElement: nnz/p, remainder to the lowest ranks        (NonZeroElement.cpp:24-39) */
SMFV_API void smfv_partition_nnz(int64_t nnz, int p, int r, int64_t *start, int64_t *end);

/* ---- single-device SpMM ------------------------------------------------- */
/* Merge-path geometry of SMFV_NONZERO over nrows rows / nnz non-zeros
 * (host): out[0] merge items (rows + non-zeros), [1] items per team, [2]
 * teams.  Team t walks diagonals [t * out[1], (t + 1) * out[1]); a row open at
 * a team boundary is finished by the carry fix-up (tests sample those rows). */
SMFV_API int smfv_merge_geometry(int nrows, int64_t nnz, int K, int64_t out[3]);

/* Device workspace (bytes) smfv_spmm_csr_f64 needs for `variant`; 0 for all
 * but SMFV_NONZERO (merge-path carry slots). */
SMFV_API int smfv_spmm_workspace_bytes(int variant, int m, int64_t nnz, int K, size_t *bytes);

/* Y = A * X on the current device.  `workspace` may be NULL when the
 * workspace size is 0. */
SMFV_API int smfv_spmm_csr_f64(int variant, int m, int n, int64_t nnz,
                               const int *d_row_ptr, const int *d_col_idx, const double *d_values,
                               const double *d_X, int64_t ldx, int K,
                               double *d_Y, int64_t ldy,
                               void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- plans: analysed once per (matrix pattern, K), executed many times --
 * The plan owns all device workspace (merge-path carries for NONZERO) and,
 * with K a multiple of 32 (or K = 4, 8, 16: one narrow column window, e.g. a
 * ColumnWise rank's K/p panel; the kernel stages and stores only the window's
 * columns, X and Y 16-byte aligned with even strides), a clustered
 * row-tile analysis of the pattern (h_col_idx needed): tiles of <= 64 rows
 * grown by adjacency whose distinct X rows (<= 239) fit a 60 KiB LDS image,
 * with a tile-ordered copy of the values and 16-bit X-row offsets.  The tiled
 * kernel (one warp-specialised block per CU, double-buffered LDS-DMA staging)
 * stages each tile's X rows once and reads them from LDS -- same per-row
 * order and arithmetic, bit-identical result; rows over a cap alone are
 * gathered straight from X by a second launch.  Tiling is used when the
 * re-use (non-zeros per staged X row) is >= 3 -- estimated first on 128 tiles
 * grown in the full pattern, so the decision does not depend on the row
 * numbering -- or when SMFV_PLAN_FORCE_TILES is set.  A NONZERO plan over
 * whole rows takes the same tiled kernel under the same rule (bit-identical
 * to the reference's NonZeroElement with one rank, which sums every row in
 * CSR order); otherwise, and with SMFV_PLAN_NO_TILES, it runs the merge path.
 * With K == 1 (SpMV) a plan over whole rows takes the chunk layout of
 * k_spmv_chunks wherever the pattern fits it (smfv_spmv_chunks_analyse):
 * consecutive rows packed into 1,024-entry chunks at fixed addresses, the
 * values snapshot and 16-bit column offsets (10 B per entry against CSR's
 * 12; 32-bit columns where a row spans more than 65,535 columns); it is a
 * tiled plan for the values contract below.
 *
 * Values contract of a TILED plan: smfv_plan_bind_values gathers a snapshot
 * of A's device values (tile order, and the directly-gathered rows) and the
 * plan computes with that snapshot until the next bind.  After the values
 * change -- at the same address or not -- the caller must bind again;
 * execute refuses a d_values pointer other than the bound one.  Untiled plans
 * read the live values.  The pattern (row_ptr / col_idx) must not change over
 * a plan's life.
 *
 * Streams: create allocates device memory and synchronises; bind and execute
 * are asynchronous and graph-capturable.  An execute on a stream other than
 * the bind's waits for the bind's gather (hipStreamWaitEvent; while capturing
 * it requires the gather to have completed).  A capture of an execute while
 * the gather is still running on another stream is refused with
 * SMFV_ERR_INVALID before anything is launched; the caller's capture, of any
 * capture mode, stays valid (the library asks for the gather's state in the
 * relaxed mode), and after the bind's stream has been synchronised the same
 * plan captures.  A bind issued while its stream is capturing becomes part of
 * the graph: the gather runs at every replay, from the values the array holds
 * then, while the plan counts those values as bound from the capture on.  An
 * execute captured after it on the same stream is ordered by the graph; an
 * eager execute with the values the graph bound last is accepted, and it is
 * the caller who orders it after a replay (the replay's stream, an event or a
 * synchronize), as for any work that follows a graph launch.  A plan is not
 * thread-safe. */
typedef struct smfv_plan_s *smfv_plan_t;
#define SMFV_PLAN_NO_TILES 1
#define SMFV_PLAN_FORCE_TILES 2
/* Opt-in: the tiled kernel sums each term with one fused multiply-add
 * instead of the reference's separate multiply and add.  Same per-row order;
 * results differ from the reference by rounding only (well inside the 1e-6
 * relative tolerance) and are no longer bit-identical. */
#define SMFV_PLAN_FMA 4
/* Tiles are seeded at the oldest unassigned neighbour of the tiles built so
 * far (a wavefront through the pattern's graph: neighbouring tiles run
 * together on one XCD and share X rows in its L2, whatever the row
 * numbering).  This flag seeds them in row order instead (A/B). */
#define SMFV_PLAN_NATURAL_SEEDS 8
/* Opt-in (BASELINE config 3's "MFMA K-panel", kept as a measured
 * alternative): the tiles run as dense 16 x 4 blocks of A on
 * v_mfma_f64_16x16x4f64 (k_rows_mfma).  Sums are reassociated by the MFMA:
 * within tolerance, not bit-identical.  The MFMA plan requires a finite X:
 * the dense blocks' zeros multiply every staged X row, so an inf or NaN in X
 * row c turns the rows of any 16-row group that uses c into NaN, also those
 * that do not reference c (every other plan keeps them finite). */
#define SMFV_PLAN_MFMA 16
/* Opt-in (measured slower, kept for A/B): the tiled plan cuts the first
 * tile of each of the kernel's blocks in two and runs the halves first and
 * last, halving the unoverlapped staging of a block's first tile and the
 * unoverlapped compute of its last -- at the cost of one more unit per block
 * (26.5 -> 27.2 us on the cop20k surrogate, K = 32). */
#define SMFV_PLAN_SPLIT_ENDS 32
/* Each XCD has its own L2, so the tiled plan splits the rows into 8 parts
 * of equal non-zero count -- row ranges, or shares of the rows' breadth-first
 * order, whichever reads fewer X rows summed over the parts -- tiles each
 * part as its own wavefront and runs part x on XCD x.  This flag keeps one
 * wavefront over the whole pattern cut into 8 consecutive shares (A/B). */
#define SMFV_PLAN_ONE_WAVEFRONT 64
/* Untiled, and the simplest row kernel for any K (one double per lane,
 * k_rows): an independent computation of the same per-row sums, used by the
 * C++ drop-in for the sequential function -- the result the parallel
 * variants are checked against (SC/main.cpp:184) -- so that check does not
 * compare a kernel with itself.  Ignored for SMFV_NONZERO. */
#define SMFV_PLAN_SIMPLE_ROWS 128
/* RETIRED (ignored): column-streamed tiles (k_rows_cs), measured 3.4x slower
 * than k_rows_ws (profiles/r03/ab_s2/); the r2-r4 lab build that kept it was
 * removed in r5.  The value stays reserved. */
#define SMFV_PLAN_CS 256
/* The tiled kernel k_rows_ws (~60-row tiles whose whole X union sits in
 * LDS), asked for explicitly (with a geometry flag below: A/B). */
#define SMFV_PLAN_WS 512
/* (r4) The geometry of k_rows_ws (A/B; without either flag the library's
 * default): GEOM1 one 1024-lane block per CU (8 compute + 8 loader waves,
 * tiles of <= 64 rows and <= 239 staged X rows, 158 KiB of LDS); GEOM2 two
 * independent 512-lane blocks per CU (4 + 4 waves, tiles of <= 32 rows and
 * <= 125 X rows, 80 KiB of LDS each), so one block's per-tile hand-off hides
 * behind the other's work.  Same per-row order: bit-identical either way.
 * Without a flag a plan takes GEOM1, except a SMALL plan (fewer than 1.5
 * GEOM1 tiles per CU, e.g. a rank's row block at p = 8), which takes GEOM2
 * when its 32-row tiles keep the re-use and add no direct rows: there one
 * unit per block is all fill and drain, and half-size units halve it
 * (7.9 -> 7.1 us on a cop20k rank block).  On whole cop20k GEOM2 is slower
 * (2.6x the units: profiles/r04/ab_geom). */
#define SMFV_PLAN_WS_GEOM1 1024
#define SMFV_PLAN_WS_GEOM2 2048
/* (r4) GEOM3: one 768-lane block per CU, 8 compute + 4 loader waves (16 X
 * pieces each), 64-row tiles: 3 waves per SIMD, so the compute waves may hold
 * up to 168 VGPRs (deeper LDS read-ahead). */
#define SMFV_PLAN_WS_GEOM3 4096
/* (r5) Live values: the tiled kernel's loaders DMA each row's value pairs
 * straight from the caller's CSR values (no snapshot, no bind pass: a bind is
 * a no-op and every execute reads the values it is given, like an untiled
 * plan).  Bit-identical to the snapshot path.  Tiled k_rows_ws plans only
 * (K = 1 chunk plans and SMFV_PLAN_MFMA keep their snapshot). */
#define SMFV_PLAN_LIVE_VALUES 8192
/* (r5) Row pairs: a k_rows_ws tile may hold up to twice its teams in rows,
 * the shortest rows riding as second rows of the teams of the next shortest
 * (a team sums its first row, stores it, then sums its second; no pair runs
 * more than one batch of 8 past the tile's longest row), with a larger entry
 * cap (2,048 against 1,792), so the tiles of short-row patterns stop at the
 * X-row cap instead of the row count.  Same per-row order: bit-identical.
 * Without either flag a plan builds both and keeps the one whose busiest
 * block runs fewer tiles (ties: one row per team): the irregular cop20k
 * stand-in pairs (10 -> 8 rounds, 27.6 -> 25.7 us), the stencil one does not
 * (8 rounds either way, and bigger tiles make longer units).  SINGLE_ROWS
 * forces one row per team, ROW_PAIRS forces pairs (A/B, tests). */
#define SMFV_PLAN_SINGLE_ROWS 16384
#define SMFV_PLAN_ROW_PAIRS 32768
/* The plan will be executed with smfv_plan_execute_axpby (below), which
 * returns SMFV_ERR_INVALID for a plan without this flag; smfv_plan_execute is
 * unaffected by it.  Create chooses the form of the epilogue
 * (smfv_plan_epilogue_mode).  AXPBY_TWO_PASS forces the two-pass form (A/B
 * runs and tests) and implies AXPBY. */
#define SMFV_PLAN_AXPBY 65536
#define SMFV_PLAN_AXPBY_TWO_PASS 131072
/* Y = A^T X.  Accepted by smfv_plan_create only.  With it a plan created from
 * the CSR of A (m x n; h_row_ptr and h_col_idx both required) computes
 * Y[n x K] = A^T X[m x K]: what BiCG, QMR, LSQR / LSMR, the normal equations
 * and the restriction of a multigrid prolongation need beside A X, from the
 * one CSR the caller holds.  No atomics: create transposes the PATTERN once on
 * the host (smfv_csr_transpose: a stable counting sort) and the plan runs the
 * row kernels of this library on it.
 *
 * Order of summation: Y[c, :] starts from s = 0.0, then s = s + values[j] *
 * X[row(j), :] over all CSR indices j with col_idx[j] == c, in ascending j,
 * multiply and add rounded separately -- the reference's sequential loop
 * (SC/SparseMatrixFatVectorMultiply.cpp:17-27) on the CSR of A^T obtained by
 * a stable counting sort of A's entries by column.  Repeated columns inside a
 * row of A stay in their CSR order; a column with no entry gives +0.0, and it
 * is written.  SEQUENTIAL / ROWWISE / COLUMNWISE: bit-identical to that loop,
 * NaN for NaN and the sign of zero included.  NONZERO: |Y - Yref| <= 1e-12 *
 * sum|a||x| + 1e-300 elementwise, and bit-identical where its inner plan takes
 * the tiled kernel, as without the flag.  SMFV_PLAN_FMA / SMFV_PLAN_MFMA keep
 * their documented looser contracts.
 *
 * Execute: d_X is m x K, d_Y is n x K; d_row_ptr / d_col_idx are ignored and
 * may be NULL (the plan owns the transposed pattern); d_values is A's values
 * array in A's order.
 *
 * Values contract: EVERY transposed plan computes from a plan-owned copy of
 * the values in transposed order, written by smfv_plan_bind_values
 * (k_permute_vals, then the inner plan's own gather from that copy) -- untiled
 * and SMFV_PLAN_LIVE_VALUES plans too ("live" then means that the tiled
 * kernel DMAs from that copy, with no tile snapshot).  So every transposed
 * plan must be bound after the values change, and a bind is never a no-op.
 * Execute refuses with SMFV_ERR_INVALID, before anything is launched, a
 * d_values other than the bound pointer and an execute before any bind.
 *
 * Streams: as for tiled plans (above): bind and execute are asynchronous and
 * capturable, a bind captured into a graph re-gathers at every replay, an
 * execute on a stream other than the bind's waits for the bind, and while
 * capturing the in-flight check is made in the relaxed mode and leaves the
 * caller's capture valid.
 *
 * With SMFV_PLAN_AXPBY: Y <- alpha A^T X + beta Y by smfv_plan_execute_axpby,
 * the formula, the beta == 0 rule and fused against two-pass exactly as
 * documented there; smfv_plan_epilogue_mode reports the inner plan's mode.
 * All other flags act on the transposed pattern (tiles on / off / forced,
 * geometries, row pairs, seeds, XCD parts, FMA, MFMA, SIMPLE_ROWS).
 * smfv_plan_stats reports the inner plan's figures, [4] including the
 * transposed pattern, permutation and values, [8] the transposition.
 *
 * Refused with SMFV_ERR_INVALID and a message, before any device allocation:
 * the flag in smfv_plan_create_rows and in every smfv_dist_plan_create*; a
 * NULL h_row_ptr or h_col_idx; a column index outside [0, n).
 *
 * Out of scope: the plan-less smfv_spmm_* family, row-block and distributed
 * plans, the C++ drop-in and the CLI (the reference has no such call),
 * bench.py, and half-stored symmetric matrices (A^T of the stored half is not
 * the other half's product). */
#define SMFV_PLAN_TRANSPOSE 262144
SMFV_API int smfv_plan_create(smfv_plan_t *plan, int variant, int m, int n, int64_t nnz,
                              const int *h_row_ptr, const int *h_col_idx, int K, int flags);
/* Plan of the row block [row_begin, row_end) of a CSR matrix (h_row_ptr /
 * h_col_idx: host arrays of the WHOLE matrix; the analysis runs on the
 * block's own rows): what one rank of SC/...RowWise.cpp:36-50 computes.
 * Execute takes the whole matrix's device arrays and writes the block's rows
 * to d_Y (row i of the block at d_Y + i * ldy), as smfv_spmm_rowblock_f64. */
SMFV_API int smfv_plan_create_rows(smfv_plan_t *plan, int variant, int row_begin, int row_end, int n,
                                   const int *h_row_ptr, const int *h_col_idx, int K, int flags);
/* Host threads a plan analysis started on the CALLING thread may use (the
 * tile analysis runs its 8 XCD parts in parallel): 0 = the default (up to 8);
 * a library building plans in the background lowers it so the caller's own
 * work keeps its cores. */
SMFV_API void smfv_set_analysis_threads(int threads);
SMFV_API int smfv_plan_bind_values(smfv_plan_t plan, const double *d_values, void *stream);
/* Host-only diagnostic: run the clustered tile analysis and build the tiled
 * kernel's plan, verify the invariants the kernel relies on (every row in
 * exactly one tile or the direct list, caps, CSR order inside rows, union
 * positions, pads on the zero row -- by replaying the kernel's reads) and
 * report out[0] tiles, [1] staged X rows, [2] re-use, [3] direct rows,
 * [4] tile entries (incl. pads), [5] non-zeros in tiles.  No device needed. */
SMFV_API int smfv_plan_analyse(int m, int n, const int *h_row_ptr, const int *h_col_idx,
                               double out[6]);
/* The same for the row block [row_begin, row_end) with the caps a plan of
 * these flags uses (smfv_plan_create_rows; (r5) SMFV_PLAN_LIVE_VALUES builds
 * and verifies the live-values layout): out[0..5] as above, [6] XCD
 * parts (8 or 1), [7] X footprint of the 8 parts (-1: not computed),
 * [8] X footprint of the plan's 8 XCD tile ranges (distinct X rows each
 * reads, summed, over the block's distinct X rows).  No device needed. */
/* (r5) The narrow-team plan of a kw = 4 / 8 column window (k_rows_wsn) for
 * the row block [row_begin, row_end), built and verified on the host (the
 * kernel's reads replayed): out[0] tiles, [1] staged X rows, [2] re-use,
 * [3] direct rows, [4] rows of the fullest tile, [5] padded entries; (r6)
 * the modelled LDS cycles of the kernel's X reads (ds_read_b128 lane groups,
 * one cycle each when conflict-free, plus one per extra distinct address on a
 * bank): [6] lane groups (the conflict-free count), [7] cycles with the
 * plan's bank-coloured image slots, [8] cycles with first-use slots.  No
 * device needed.  (SC/...ColumnWise.cpp:34-48 on a rank's K/p panel.) */
SMFV_API int smfv_wsn_plan_analyse(int row_begin, int row_end, int n, const int *h_row_ptr,
                                   const int *h_col_idx, int kw, double out[9]);
SMFV_API int smfv_plan_analyse_rows(int row_begin, int row_end, int n, const int *h_row_ptr,
                                    const int *h_col_idx, int flags, double out[9]);
/* The K = 1 chunk layout (k_spmv_chunks) of the row block [row_begin,
 * row_end) with `cap` entry slots per chunk (512, 1024 or 2048; 0: the plans'
 * default), built and verified as smfv_plan_create builds it for K = 1:
 * out[0] 1 if the pattern fits the layout (else 0: a row longer than a
 * chunk), [1] chunks, [2] non-zeros placed, [3] most rows in a chunk, [4]
 * mean fill of a chunk's slots, [5] 1 for the wide layout (32-bit columns:
 * some row spans more than 65,535 columns), 0 for 16-bit offsets.  No device
 * needed.  (SC/SparseMatrixFatVectorMultiply.cpp:17-27 at vecCols = 1.) */
SMFV_API int smfv_spmv_chunks_analyse(int row_begin, int row_end, int n, const int *h_row_ptr,
                                      const int *h_col_idx, int cap, double out[6]);
SMFV_API int smfv_plan_execute(smfv_plan_t plan, const int *d_row_ptr, const int *d_col_idx,
                               const double *d_values, const double *d_X, int64_t ldx,
                               double *d_Y, int64_t ldy, void *stream);
/* Y <- alpha * A * X + beta * Y, in place, for a plan created with
 * SMFV_PLAN_AXPBY: the inner step of block CG, LOBPCG, Chebyshev filtering
 * and subspace iteration.  Same argument rules, values contract (bind),
 * stream ordering and error reporting as smfv_plan_execute; asynchronous on
 * the stream and graph-capturable, no allocation and no synchronisation.
 *
 * With s the row sum exactly as smfv_plan_execute computes it and y0 the
 * value in Y before the call:
 *   beta != 0:  y = fl(fl(alpha * s) + fl(beta * y0)) -- two multiplies and
 *               one add, each rounded, never contracted into an FMA
 *               (SMFV_PLAN_FMA plans included);
 *   beta == 0:  y = fl(alpha * s).  Y is NOT read: a NaN or inf in y0 does not
 *               propagate, and nothing is added, so the sign of a zero sum
 *               survives.  Hence alpha = 1, beta = 0 gives the bits of
 *               smfv_plan_execute.
 * alpha is always applied by multiplication (no shortcut for alpha == 0:
 * 0 * inf is NaN, as in IEEE).  The operation covers the plan's rows and the
 * K columns only; padding beyond K (ldy > K) is neither read nor written.
 * SEQUENTIAL / ROWWISE / COLUMNWISE: bit-identical to the formula applied to
 * the reference's sequential sums, NaN for NaN and the sign of zero
 * included.  NONZERO: |Y - Yexp| <= 1e-12 * (|alpha| * sum|a||x| + |beta| *
 * |y0|) elementwise.
 *
 * Two forms, chosen at create (smfv_plan_epilogue_mode):
 *   1 fused     the epilogue runs in the store of the kernel that computed
 *               the sum (k_rows_ws, k_rows_list, k_rows_mh, k_rows, every
 *               run-time fallback of execute included): one launch, y0 read
 *               once by the lane that overwrites it, no read at beta == 0.
 *               SEQUENTIAL / ROWWISE / COLUMNWISE plans with K >= 2 that are
 *               not SMFV_PLAN_FMA, SMFV_PLAN_MFMA or k_rows_wsn plans.
 *   2 two-pass  everything else (K = 1, every NONZERO plan -- its kernels
 *               store partial sums --, FMA, MFMA, k_rows_wsn) and any plan
 *               with SMFV_PLAN_AXPBY_TWO_PASS: the plan's own launches into a
 *               plan-owned scratch of m x K doubles (allocated at create,
 *               counted in the plan's device bytes), then one k_axpby pass.
 * Out of scope: distributed plans (the flag passes through to the rank-local
 * plan harmlessly; no smfv_dist_plan_* axpby execute exists), the plan-less
 * smfv_spmm_csr_f64 family, the C++ drop-in and the CLI (the reference has no
 * such call), and bench.py. */
SMFV_API int smfv_plan_execute_axpby(smfv_plan_t plan, const int *d_row_ptr, const int *d_col_idx,
                                     const double *d_values, const double *d_X, int64_t ldx,
                                     double alpha, double beta, double *d_Y, int64_t ldy, void *stream);
/* *mode = 0 (no epilogue: the plan lacks SMFV_PLAN_AXPBY), 1 (fused) or 2
 * (two-pass). */
SMFV_API int smfv_plan_epilogue_mode(smfv_plan_t plan, int *mode);
/* out[0] tiled (0/1), [1] tiles, [2] staged X rows per panel, [3] re-use
 * (tiled non-zeros / staged rows), [4] plan device bytes, [5] direct rows,
 * [6] first row of the block, [7] re-use estimated on the sample tiles (-1:
 * not sampled), [8] host analysis + upload time (ms), [9] values gathered
 * by each bind (snapshot entries, pads included), [10] 1 if the tiles run on
 * the MFMA kernel (SMFV_PLAN_MFMA), [11] XCD parts (8: one part of the
 * rows per XCD, 1: one wavefront), [12] X rows the 8 parts read, summed,
 * over the pattern's X rows (-1: not computed), [13] the kernel a tiled
 * plan runs: 0 none (untiled), 1 k_rows_ws, 2 k_rows_mfma, 3 k_spmv_chunks,
 * (r5) 5 k_rows_wsn (narrow-team tiles of a K = 4 / 8 window),
 * (4 was the retired k_rows_cs); [14] (r5) 1 if the tiled plan reads live
 * values (SMFV_PLAN_LIVE_VALUES), else 0; [15] (r4) the k_rows_ws
 * geometry (1: one 1024-lane block per CU, 2: two 512-lane blocks, 3: one
 * 768-lane block; 0 other); [16] (r4) 1 if a bind writes the snapshot's real
 * entries from bind items of up to 4 consecutive non-zeros (pads written once
 * at create: k_bind_items), 0 if it gathers every entry by index; [17] (r5)
 * rows summed as a team's second row (SMFV_PLAN_SINGLE_ROWS) */
#define SMFV_PLAN_STATS 18
SMFV_API int smfv_plan_stats(smfv_plan_t plan, double out[SMFV_PLAN_STATS]);
/* *flag = 1 for a plan created with SMFV_PLAN_TRANSPOSE, else 0. */
SMFV_API int smfv_plan_is_transposed(smfv_plan_t plan, int *flag);
/* The CSR pattern of A^T (n rows, m columns) from the CSR pattern of A (m x
 * n), as SMFV_PLAN_TRANSPOSE plans build it: a stable counting sort of A's
 * entries by column, O(nnz + m + n), on the host (no device needed).
 * t_row_ptr[n + 1]; for transposed entry j, t_col_idx[j] is its row in A and
 * t_perm[j] its CSR index in A (values of A^T: values[t_perm[j]]), ascending
 * inside every transposed row.  Every column index is validated before it is
 * used (SMFV_ERR_INVALID for one outside [0, n), or a row_ptr that does not
 * start at 0 or decreases), and the result is verified by replay before it is
 * returned. */
SMFV_API int smfv_csr_transpose(int m, int n, const int *h_row_ptr, const int *h_col_idx, int *t_row_ptr,
                                int *t_col_idx, int *t_perm);
SMFV_API int smfv_plan_destroy(smfv_plan_t plan);

/* ---- triangular solves: T Y = X with a fat right-hand side ----------------
 * The preconditioner step of the block Krylov methods the plans above serve
 * (Gauss-Seidel / SSOR sweeps, ILU(0) / IC(0) factors, multigrid smoothers).
 * T is the lower triangle (SMFV_TRSM_UPPER: the upper) of a square m x m CSR
 * matrix the caller already holds; X and Y are m x K, row-major, ldx, ldy >=
 * K, fp64.  No atomics, a fixed launch sequence, the same bits on every run.
 *
 * Semantics.  A lower solve takes the rows i = 0 .. m-1; an upper solve
 * mirrors it (rows descend, the strict entries are those with c > i).  For
 * every column k:
 *     s = X[i,k]
 *     for j in row i's CSR entries, ascending j:   c = col_idx[j]
 *         c <  i : s = fl(s - fl(values[j] * Y[c,k]))   separate multiply and
 *                                                       subtract, never an FMA
 *         c == i : d = values[j] for the first such entry,
 *                  d = fl(d + values[j]) for each later one
 *         c >  i : ignored (the other triangle)
 *     Y[i,k] = fl(s / d)      a true IEEE division, not a reciprocal multiply
 *     Y[i,k] = s              SMFV_TRSM_UNIT_DIAG: entries with c == i are
 *                             ignored too
 * The result is bit-identical to this sequential substitution, NaN for NaN
 * and the sign of zero included; NaN, inf, signed zeros and subnormals
 * propagate exactly as in the loop.
 *   - The whole matrix is accepted: the other triangle is ignored, so with A
 *     itself `lower` is the forward Gauss-Seidel sweep (D + L)^-1 X and
 *     `upper` the backward one.
 *   - Unsorted rows and repeated columns are legal: repeated strict entries
 *     each subtract, in CSR order; repeated diagonal entries are summed in CSR
 *     order.
 *   - A zero or non-finite pivot gives what IEEE gives (+-inf, NaN), written
 *     without any check or synchronisation.
 *   - In place: d_Y == d_X with ldy == ldx is allowed (each element is read
 *     and written by the same lane); any other overlap is undefined.
 *   - Columns beyond K (padding) are neither read nor written.
 *   - T^T Y = X (the second half of IC) is not a flag: smfv_csr_transpose
 *     gives the caller the CSR of the other triangle (values: values[t_perm]),
 *     and a plan of that solves it.
 *   - Out of scope: distributed plans, the C++ drop-in, the CLI, bench.py.
 *
 * Refused at create with SMFV_ERR_INVALID and a message, before any device
 * allocation: a row with no diagonal entry without SMFV_TRSM_UNIT_DIAG (the
 * message names the first such row), a column index outside [0, m), K < 1,
 * NO_CHAIN together with CHAIN_ALL, unknown flag bits.
 *
 * Execution is level-scheduled: level(i) = 1 + the highest level
 * among the rows that row i's strict entries name.  A level of more than
 * `thin` rows is one grid launch (k_trsm_level); a maximal run of consecutive
 * levels of <= thin rows is one launch of a single 1024-lane block that walks
 * them with a block barrier in between (k_trsm_chain).  A dependency crosses
 * between workgroups only at a kernel boundary: no flags, no spinning, no
 * cooperative launch.  The schedule never changes the arithmetic: every
 * setting below gives the same bits.
 *
 * Values contract (that of the transposed plans): bind copies A's values
 * into plan order (k_permute_vals) and writes each row's pivot d; the plan
 * computes from that copy until the next bind, so bind again after the values
 * change.  Execute refuses with SMFV_ERR_INVALID, before anything is
 * launched, a plan never bound and a d_values other than the bound pointer.
 * The pattern must not change over a plan's life.
 *
 * Streams (as for tiled plans): create allocates device memory and
 * synchronises; bind and execute are asynchronous and graph-capturable -- no
 * allocation, no synchronisation, no host read-back.  An execute on a stream
 * other than the bind's waits for the bind; while capturing, the bind must
 * have completed, which is asked in the relaxed capture mode, so a refusal
 * leaves the caller's capture valid.  A bind captured into a graph gathers
 * again at every replay.  A plan is not thread-safe. */
typedef struct smfv_trsm_plan_s *smfv_trsm_plan_t;
#define SMFV_TRSM_UPPER 1      /* default: lower */
#define SMFV_TRSM_UNIT_DIAG 2
#define SMFV_TRSM_NO_CHAIN 4   /* every level its own launch (A/B, tests) */
#define SMFV_TRSM_CHAIN_ALL 8  /* all levels in the one-block kernel, one launch (A/B, tests) */
/* A/B: a thin level is one of <= r rows (1..65535; 0 = the library's default,
 * out[11] below) */
#define SMFV_TRSM_THIN_ROWS(r) (((r) & 0xffff) << 8)
/* out[0] levels, [1] rows of the widest level, [2] launches per execute,
 * [3] chain launches, [4] rows solved by chain launches, [5] most levels in
 * one chain launch, [6] strict entries used, [7] entries ignored (the other
 * triangle; with UNIT_DIAG the diagonal too), [8] diagonal entries, [9] plan
 * device bytes (0 from smfv_trsm_analyse), [10] analysis ms, [11] the
 * thin-level threshold in rows */
#define SMFV_TRSM_STATS 12
SMFV_API int smfv_trsm_plan_create(smfv_trsm_plan_t *plan, int m, int64_t nnz, const int *h_row_ptr,
                                   const int *h_col_idx, int K, int flags);
SMFV_API int smfv_trsm_plan_bind_values(smfv_trsm_plan_t plan, const double *d_values, void *stream);
SMFV_API int smfv_trsm_plan_execute(smfv_trsm_plan_t plan, const double *d_values, const double *d_X, int64_t ldx,
                                    double *d_Y, int64_t ldy, void *stream);
SMFV_API int smfv_trsm_plan_stats(smfv_trsm_plan_t plan, double out[SMFV_TRSM_STATS]);
SMFV_API int smfv_trsm_plan_destroy(smfv_trsm_plan_t plan);
/* Host only: the analysis of smfv_trsm_plan_create (levels, layout, schedule,
 * verified by replay) and its figures, with the same refusals.  No device
 * needed. */
SMFV_API int smfv_trsm_analyse(int m, const int *h_row_ptr, const int *h_col_idx, int K, int flags,
                               double out[SMFV_TRSM_STATS]);
/* Host only: level[i] (1-based) of every row, order[p] the row at plan
 * position p (rows by level, ascending row index inside a level) and the
 * level count.  Only SMFV_TRSM_UPPER of `flags` matters (diagonal entries
 * never set a level).  SMFV_ERR_INVALID for a column outside [0, m). */
SMFV_API int smfv_trsm_levels(int m, const int *h_row_ptr, const int *h_col_idx, int flags, int *level, int *order,
                              int *nlevels);

/* ---- ILU(0): the factors the triangular solves above apply ----------------
 * Input: a square m x m CSR pattern (row_ptr, col_idx, int32) and fp64 values
 * a in CSR order.  Output: f, nnz doubles in the same CSR order; the
 * strict-lower entries of f are L (unit diagonal, not stored), the diagonal
 * and strict-upper entries are U.  No atomics, a fixed launch sequence.
 *
 * Semantics.
 *     for i = 0 .. m-1:
 *         w[j] = a[j] for every CSR entry j of row i
 *         for every strict-lower entry p of row i, in ASCENDING COLUMN
 *                                   k = col_idx[p] (not in CSR order):
 *             w[p] = fl(w[p] / f[diag(k)])      a true IEEE division, never a
 *                                               reciprocal multiply
 *             for every entry q of row k with col_idx[q] > k:
 *                 if row i has an entry r with col_idx[r] == col_idx[q]:
 *                     w[r] = fl(w[r] - fl(w[p] * f[q]))   separate multiply
 *                                               and subtract, never an FMA
 *         f[j] = w[j] for every entry j of row i
 * Row k is final before row i uses it; entries of row k outside row i's
 * pattern are dropped (zero fill-in).  Each w[r] is updated once per step k,
 * in ascending k, and the order of the q inside a step does not touch the
 * arithmetic, so the result is a function of the input alone: it is
 * bit-identical to this loop, NaN for NaN and the sign of zero included, on
 * every run and with every schedule setting below.
 *   - Unsorted rows are legal: the elimination order is by column, the
 *     output stays in the caller's CSR order.
 *   - A zero or non-finite pivot gives what IEEE gives (+-inf, NaN), written
 *     without any check, read-back or synchronisation.
 *   - In place: d_F == d_values is allowed (row i is read before it is
 *     written, and other rows read only earlier rows of f); any other overlap
 *     is undefined.
 *   - The result plugs into the solves above: a trsm plan of f's pattern with
 *     SMFV_TRSM_UNIT_DIAG (lower: L, f's diagonal ignored), then one with
 *     SMFV_TRSM_UPPER (U, exactly one diagonal entry per row), apply
 *     U^-1 L^-1.
 *   - Out of scope: IC(0), ILU(k) and threshold variants, pivot shifting or
 *     repair, distributed plans, the C++ drop-in, the CLI, bench.py.
 *
 * Refused at create with SMFV_ERR_INVALID and a message, before any device
 * allocation: a row with no diagonal entry (the message names the first such
 * row), a column repeated inside a row (ILU(0) of a pattern with duplicates
 * has no agreed meaning; the message names row and column), a column index
 * outside [0, m), a row_ptr that does not start at 0 or decreases, unknown
 * flag bits, NO_CHAIN together with CHAIN_ALL, an update list of 2^31 pairs
 * or more.
 *
 * Execution.  Row i needs exactly the rows its strict-lower
 * entries name, so the levels, the order of the rows and the schedule are
 * those of the lower solve (smfv_trsm_levels with flags = 0): a level of more
 * than `thin` rows is one grid launch (k_ilu0_level, a wavefront per row, its
 * working values in a slot of 256 doubles of LDS: 8,192 bytes per 256-lane
 * block), a maximal run of consecutive thinner levels one launch of a single
 * 1024-lane block with a block barrier between levels (k_ilu0_chain, 32,768
 * bytes of LDS).  A row of more than 256 entries is a LONG row and is
 * eliminated by a whole block, in d_F itself, with a block barrier between
 * its steps; rows of any length work.  A dependency crosses between
 * workgroups only at a kernel boundary: no flags, no spinning, no atomics, no
 * cooperative launch.
 *
 * Streams: create allocates device memory and synchronises.  factor is
 * asynchronous and graph-capturable -- no allocation, no synchronisation, no
 * host read-back -- and reads d_values when it runs: the plan holds no values
 * and has no bind.  The pattern must not change over a plan's life.  A plan
 * is not thread-safe. */
typedef struct smfv_ilu0_plan_s *smfv_ilu0_plan_t;
#define SMFV_ILU0_NO_CHAIN 4   /* every level its own launch (A/B, tests) */
#define SMFV_ILU0_CHAIN_ALL 8  /* all levels in the one-block kernel, one launch (A/B, tests) */
/* A/B: a thin level is one of <= r rows (1..65535; 0 = the library's default,
 * out[14] below) */
#define SMFV_ILU0_THIN_ROWS(r) (((r) & 0xffff) << 8)
/* out[0] levels, [1] rows of the widest level, [2] launches per
 * factorisation, [3] chain launches, [4] rows in chain launches, [5] most
 * levels in one chain launch, [6] steps (strict-lower entries), [7] update
 * pairs, [8] most steps in a row, [9] most pairs in a row, [10] long rows,
 * [11] LDS slot entries, [12] plan device bytes (0 from smfv_ilu0_analyse),
 * [13] analysis ms, [14] the thin-level threshold in rows */
#define SMFV_ILU0_STATS 15
SMFV_API int smfv_ilu0_plan_create(smfv_ilu0_plan_t *plan, int m, int64_t nnz, const int *h_row_ptr,
                                   const int *h_col_idx, int flags);
SMFV_API int smfv_ilu0_plan_factor(smfv_ilu0_plan_t plan, const double *d_values, double *d_F, void *stream);
SMFV_API int smfv_ilu0_plan_stats(smfv_ilu0_plan_t plan, double out[SMFV_ILU0_STATS]);
SMFV_API int smfv_ilu0_plan_destroy(smfv_ilu0_plan_t plan);
/* Host only: the analysis of smfv_ilu0_plan_create (levels, symbolic phase,
 * schedule, verified by replay) and its figures, with the same refusals.  No
 * device needed. */
SMFV_API int smfv_ilu0_analyse(int m, const int *h_row_ptr, const int *h_col_idx, int flags,
                               double out[SMFV_ILU0_STATS]);

/* ---- Multicolour reordering: fewer levels for the solves and ILU(0) --------
 * The solves and the factorisation above cost a fixed time per LEVEL of the
 * triangle's dependency graph, whatever the schedule does; only another
 * numbering of the matrix removes levels.  This family gives an ordering, the
 * renumbered CSR and the device kernels that carry values and fat vectors
 * into the new numbering and back.  No existing plan changes: the renumbered
 * matrix B is an ordinary CSR for every plan family of this header.
 *
 * A multicolour ILU(0) is a DIFFERENT, usually somewhat weaker, preconditioner
 * than the natural-order one (the standard trade on GPUs): the factors of B
 * are not a renumbering of the factors of A.
 *
 * The ordering (smfv_order_multicolor; host only, no device needed; the values
 * are not looked at).  The rule is fixed, so a caller can reproduce it:
 *   - the graph is the pattern of A + A^T without the diagonal (A^T by
 *     smfv_csr_transpose); repeated columns, unsorted rows and empty rows are
 *     legal;
 *   - rows are coloured in the order i = 0 .. m-1;
 *   - color[i] is the smallest c >= 0 that no already-coloured neighbour
 *     holds (only neighbours j < i can hold a colour): first-fit greedy;
 *   - *ncolors = max + 1, and 0 for m = 0;
 *   - perm lists the rows sorted by (color, i), a stable sort: new row i' is
 *     old row perm[i'].
 *   Consequence: in the renumbered matrix two rows of one colour never couple,
 *   so its lower and its upper triangle each have at most *ncolors levels
 *   (smfv_trsm_analyse, smfv_ilu0_analyse report them).
 *   h_color may be NULL.  Refused with SMFV_ERR_INVALID and a message: a
 *   column outside [0, m), a row_ptr that does not start at 0 or decreases,
 *   unknown flag bits (none are defined: flags must be 0), NULL outputs.
 *
 * The renumbering (smfv_csr_permute_sym; host only).  B = P A P^T: row i' of
 * B is row h_perm[i'] of A and a column c becomes inv[c] (inv the inverse of
 * h_perm).  THE ENTRIES OF A ROW KEEP THE CALLER'S CSR ORDER; they are not
 * sorted.  Entry j' of B is entry b_vperm[j'] of A (int, nnz < 2^31, like the
 * entry map of smfv_csr_transpose).  Because the order is kept, every row of
 * B is summed in the order of the row of A it came from:
 *     B (P X) == P (A X)   bit for bit, on every bit-exact plan family.
 *   Unsorted rows are legal input to the plans, the solves and ILU(0).
 *   Refused: an h_perm that is not a permutation of [0, m) (the message names
 *   the first offending position), a malformed pattern as above, NULL
 *   outputs.
 *
 * The device plan (smfv_reorder_plan_*).  create validates both permutations
 * on the host before any device call (h_perm a permutation of [0, m), h_vperm
 * one of [0, nnz); h_vperm may be NULL with nnz = 0: a plan for rows only),
 * uploads h_perm, its inverse and h_vperm, and synchronises.
 *   values:  d_dst[j'] = d_src[vperm[j']], j' in [0, nnz)   (k_permute_vals)
 *   rows, SMFV_REORDER_TO_NEW:  Y[i', 0:K] = X[perm[i'], 0:K]
 *   rows, SMFV_REORDER_TO_OLD:  Y[r,  0:K] = X[inv[r],  0:K]
 * so TO_OLD undoes TO_NEW.  Both directions are a gather with coalesced
 * writes, by one kernel (k_permute_rows: a team of lanes covers the K columns
 * of a row, several rows per wavefront and four rows in flight per team;
 * 16-byte accesses when X, Y, ldx, ldy and K allow them, 8-byte otherwise;
 * 64-bit element offsets).  Bit patterns are moved, not numbers: NaN payloads
 * and the sign of zero survive.  Only the K columns are read and written:
 * padding beyond K (ldx, ldy >= K) is neither read nor written.
 *   Refused with SMFV_ERR_INVALID, nothing launched: d_Y == d_X, K < 1, a
 *   NULL pointer, ldx < K or ldy < K, an unknown direction.  Any other
 *   overlap of X and Y is undefined.
 *   SMFV_REORDER_STORE_NT, or'ed to the direction, writes Y with non-temporal
 *   stores (A/B; plain stores are the default, profiles/reorder/README.md).
 *
 * Streams: create allocates device memory and synchronises.  values and rows
 * are asynchronous and graph-capturable -- no allocation, no synchronisation,
 * no host read-back; the plan holds no values and has no bind.  A plan is not
 * thread-safe.
 *
 * Out of scope: other orderings (largest-degree-first, RCM, nested
 * dissection), balancing the sizes of the colours, permutations fused into
 * the solve kernels, IC(0), distributed plans, the C++ drop-in, the CLI,
 * bench.py. */
typedef struct smfv_reorder_plan_s *smfv_reorder_plan_t;
#define SMFV_REORDER_TO_NEW 1   /* Y[i'] = X[perm[i']] */
#define SMFV_REORDER_TO_OLD 2   /* Y[r] = X[inv[r]] */
#define SMFV_REORDER_STORE_NT 4 /* non-temporal stores of Y (A/B) */
/* out[0] m, [1] nnz, [2] plan device bytes, [3] host validation + upload ms */
#define SMFV_REORDER_STATS 4
SMFV_API int smfv_order_multicolor(int m, const int *h_row_ptr, const int *h_col_idx, int flags, int *h_perm,
                                   int *h_color, int *ncolors);
SMFV_API int smfv_csr_permute_sym(int m, const int *h_row_ptr, const int *h_col_idx, const int *h_perm,
                                  int *b_row_ptr, int *b_col_idx, int *b_vperm);
SMFV_API int smfv_reorder_plan_create(smfv_reorder_plan_t *plan, int m, int64_t nnz, const int *h_perm,
                                      const int *h_vperm);
SMFV_API int smfv_reorder_plan_values(smfv_reorder_plan_t plan, const double *d_src, double *d_dst, void *stream);
SMFV_API int smfv_reorder_plan_rows(smfv_reorder_plan_t plan, int direction, const double *d_X, int64_t ldx, int K,
                                    double *d_Y, int64_t ldy, void *stream);
SMFV_API int smfv_reorder_plan_stats(smfv_reorder_plan_t plan, double out[SMFV_REORDER_STATS]);
SMFV_API int smfv_reorder_plan_destroy(smfv_reorder_plan_t plan);

/* ---- Block vectors: column dots and per-column scaled updates --------------
 * The pieces a preconditioned block Krylov iteration needs besides A X and
 * M^-1 X, on m x K row-major blocks with leading dimensions >= K: one dot
 * product per column in a FIXED SUMMATION ORDER, and updates Y += s X,
 * Y = X + s Y whose per-column scalars s[j] stay on the device (a quotient of
 * two earlier dots), so no host read sits between a dot and its use and a
 * whole iteration captures into a graph.  libsmfv is built with
 * -ffp-contract=off: every product and every sum below is rounded on its own,
 * there is never an FMA.
 *
 * The column-dot rule (smfv_coldot_rule returns its two constants,
 * CHUNK = 512 rows and STRANDS = 32; smfv_coldot_host is the rule in plain
 * C++).  d[j] = coldot(X, Y)[j]:
 *   - rows are cut into chunks of CHUNK consecutive rows; the last may be
 *     short;
 *   - inside chunk c, strand s (0 <= s < STRANDS) starts at +0.0 and, for
 *     t = 0, 1, ... in ascending order, adds fl(X[r,j] * Y[r,j]) for
 *     r = c*CHUNK + s + t*STRANDS while r is inside the chunk and below m;
 *   - the strands combine by the shuffle-down tree: for h = 16, 8, 4, 2, 1
 *     (STRANDS/2 downwards): v[s] = fl(v[s] + v[s+h]) for s < h; v[0] is the
 *     chunk's partial;
 *   - d[j] starts at +0.0 and adds the chunk partials in ascending chunk
 *     order.  m = 0 gives +0.0.
 *   An accumulator that starts at +0.0 never becomes -0.0, so a missing row
 *   equals a product of +0.0 (a restatement may zero-pad to a multiple of
 *   CHUNK), and no result is ever -0.0.  The result depends on (m, K, the
 *   data) only -- not on the grid, the team width, the 8- / 16-byte access
 *   path or the device.  NaN in gives NaN out (payloads are not promised),
 *   inf - inf is NaN, overflow goes to +-inf.  X may be Y.
 *   On the device: k_coldot_partial writes one partial per (chunk, column)
 *   into the caller's workspace (smfv_coldot_workspace_bytes:
 *   max(1, chunks) * K doubles; it needs no zeroing, no stale entry is ever
 *   read), k_coldot_final adds them in chunk order.  Both are launched on
 *   every call, also for m = 0.  No atomics, flags or cooperative launch: the
 *   hand-over is the kernel boundary.  Only the K columns are read.
 *
 * The scalar rule.  s[j] = fl(num[j] / den[j]), a true IEEE division;
 * d_den == NULL: s[j] = num[j].  SMFV_COL_NEGATE flips the sign of s[j]
 * (exact).  SMFV_COL_ZERO_DEN: s[j] = +0.0 wherever den[j] == 0 (either
 * zero), before the flip -- the breakdown guard of a column whose residual is
 * exactly zero; without it plain IEEE applies (x/0 = +-inf, 0/0 = NaN).
 * Every lane forms its own quotient from the device arrays.
 *   axpy:  Y[i,j] = fl(Y[i,j] + fl(s[j] * X[i,j]))
 *   xpay:  Y[i,j] = fl(X[i,j] + fl(s[j] * Y[i,j]))
 *   X may be Y (in place); any other overlap is undefined.  m = 0 launches
 *   nothing.
 *   smfv_pcg_update_f64, the fused update of a PCG iteration, in one pass over
 *   four blocks: X += s P, R += (-s) Q, then rr = coldot(R, R) on the new R.
 *   It is bit-identical to smfv_col_axpy_f64(flags) on (P, X),
 *   smfv_col_axpy_f64(flags ^ SMFV_COL_NEGATE) on (Q, R) and
 *   smfv_coldot_f64(R, R), and launches k_pcg_update and k_coldot_final on
 *   every call.
 *
 * Refused with SMFV_ERR_INVALID before any device call: K < 1, m < 0, a
 * leading dimension below K, unknown flag bits, a NULL num / out / workspace,
 * a NULL block with m > 0, and in the fused call any two of P, Q, X, R that
 * share an element (exact aliasing included).
 *
 * Streams: every call is asynchronous on `stream` and graph-capturable -- no
 * allocation, no synchronisation, no host read.
 *
 * Out of scope: dots fused into the stores of the SpMM or solve kernels,
 * other Krylov methods (Gram matrices X^T Y and a coupled block CG: the next
 * section), distributed plans, the C++ drop-in, the CLI, bench.py. */
#define SMFV_COL_NEGATE 1   /* s[j] = -s[j] (exact) */
#define SMFV_COL_ZERO_DEN 2 /* s[j] = +0.0 where den[j] == 0 */
SMFV_API int smfv_coldot_rule(int *chunk, int *strands);
SMFV_API int smfv_coldot_workspace_bytes(int m, int K, size_t *bytes);
SMFV_API int smfv_coldot_host(int m, int K, const double *h_X, int64_t ldx, const double *h_Y, int64_t ldy,
                              double *h_out);
SMFV_API int smfv_coldot_f64(int m, int K, const double *d_X, int64_t ldx, const double *d_Y, int64_t ldy,
                             double *d_out, double *d_workspace, void *stream);
SMFV_API int smfv_col_axpy_f64(int m, int K, const double *d_num, const double *d_den, int flags, const double *d_X,
                               int64_t ldx, double *d_Y, int64_t ldy, void *stream);
SMFV_API int smfv_col_xpay_f64(int m, int K, const double *d_num, const double *d_den, int flags, const double *d_X,
                               int64_t ldx, double *d_Y, int64_t ldy, void *stream);
SMFV_API int smfv_pcg_update_f64(int m, int K, const double *d_num, const double *d_den, int flags, const double *d_P,
                                 int64_t ldp, const double *d_Q, int64_t ldq, double *d_X, int64_t ldx, double *d_R,
                                 int64_t ldr, double *d_rr, double *d_workspace, void *stream);

/* ---- Coupled blocks: Gram matrices, block . matrix updates, small solves ----
 * What a true block Krylov method needs on top of the block-vector family: the
 * K x K Gram matrix of two blocks, the update of a block by another block
 * times a small matrix, and the solution of a small dense system, all on the
 * device, so that a coupled block PCG iteration makes no host read and
 * captures into a graph.  fp64, row-major with leading dimensions, never an
 * FMA (-ffp-contract=off: every product and sum is rounded on its own), no
 * atomics, flags, spinning or cooperative launch, a fixed launch sequence.
 *
 * smfv_gram_f64: G = X^T Y.  X is m x Kx, Y is m x Ky, G is Kx x Ky with
 *   ldg >= Ky, Kx and Ky each in 1..128; X may be Y.  G[i,j] is the
 *   column-dot rule of the block-vector section applied, with nothing changed,
 *   to column i of X and column j of Y: chunks of CHUNK = 512 rows,
 *   STRANDS = 32 interleaved accumulators from +0.0 adding fl(x * y) in
 *   ascending row order, the shuffle-down tree h = 16, 8, 4, 2, 1, the chunk
 *   partials added in ascending chunk order from +0.0.  So
 *   gram(X, Y)[i,j] == coldot(X[:,i], Y[:,j]) bit for bit, diag(gram(R, R))
 *   is coldot(R, R), no entry is ever -0.0, NaN in gives NaN out, m = 0 gives
 *   +0.0, and the result depends on (m, Kx, Ky, the data) only -- not on the
 *   grid, the tiling of G, the access width or the alignment path.
 *   On the device: k_gram_partial writes one Kx x Ky partial per chunk into
 *   the caller's workspace (smfv_gram_workspace_bytes: max(1, chunks) * Kx *
 *   Ky doubles; it needs no zeroing, no stale entry is ever read),
 *   k_gram_final adds them in chunk order, one lane per entry.  Both are
 *   launched on every call, also for m = 0.  smfv_gram_host is the rule in
 *   plain C++.  smfv_gram_set_tiling (tests, A/B runs) forces one of the
 *   register tilings of k_gram_partial: 0 = chosen by (Kx, Ky), 1 = 4 x 8,
 *   2 = 2 x 4, 3 = 1 x 1 accumulators per lane; the bits are the same.
 *
 * smfv_block_mul_f64: Y = Z +- X C.  X is m x Kx, C is Kx x Ky on the device
 *   with ldc >= Ky, Z and Y are m x Ky, Kx and Ky each in 1..128.  For every
 *   (i, j): acc = Z[i,j], or +0.0 when d_Z == NULL; for l = 0 .. Kx-1
 *   ascending: acc = fl(acc + fl(X[i,l] * c[l,j])); Y[i,j] = acc, where c = C,
 *   or -C under SMFV_BLOCK_NEGATE (the flip is exact).  Bit-identical to that
 *   loop, NaN and the sign of zero included.  Two aliases are legal: Y == Z
 *   (same pointer and ld), and Y == X when Kx == Ky (same pointer and ld): the
 *   kernel holds a row's X values in LDS, their loads waited for, before the
 *   row's first store.  m = 0 launches nothing; otherwise one launch,
 *   k_block_mul.
 *
 * smfv_small_solve_f64: C = G^-1 H.  G is K x K (K in 1..128, not modified),
 *   H and C are K x N (N in 1..128), all on the device with leading
 *   dimensions; C may be H (same pointer and ld).  LU without pivoting in the
 *   order of the ILU(0) section, then its two solves:
 *     factor, on a copy W of G: for i ascending and k < i ascending:
 *       W[i,k] = fl(W[i,k] / W[k,k]); for j > k:
 *       W[i,j] = fl(W[i,j] - fl(W[i,k] * W[k,j]));
 *     forward: s = H[i,n]; for k < i ascending: s = fl(s - fl(W[i,k] * T[k,n]));
 *       T[i,n] = s;
 *     backward, i descending: s = T[i,n]; for k > i ascending:
 *       s = fl(s - fl(W[i,k] * C[k,n])); C[i,n] = fl(s / W[i,i]).
 *   Divisions are true IEEE divisions; a zero or non-finite pivot gives what
 *   IEEE gives, there is no check and no read-back.  One launch of one block,
 *   k_small_solve: W in LDS, right-looking elimination with a barrier per
 *   pivot (every W[i,j] is updated once per k in ascending k, so the bits are
 *   those of the row loop), one lane per right-hand-side column for the two
 *   substitutions.  smfv_small_solve_host is the rule in plain C++.
 *
 * Refused with SMFV_ERR_INVALID before any device call: Kx, Ky, K or N outside
 * 1..128, m < 0, a leading dimension below its width, unknown flag bits, a
 * NULL output or workspace, a NULL block with m > 0 (a NULL G, H or C matrix
 * always); in block_mul, Y sharing an element with Z or X other than by the
 * two aliases above, and C sharing an element with Y; in small_solve, C
 * sharing an element with G, or with H other than by C == H.
 *
 * Streams: every call is asynchronous on `stream` and graph-capturable -- no
 * allocation, no synchronisation, no host read.
 *
 * A coupled block PCG built from these (CoupledBlockPCG in the Python package)
 * has no breakdown guard: a rank-deficient block (a zero or repeated
 * right-hand-side column, columns that become dependent) makes a Gram matrix
 * singular and the IEEE infinities and NaNs propagate.
 *
 * Out of scope: a fused "X += P a, R -= Q a, rr" pass, dots fused into the
 * SpMM stores, MFMA, deflation and the QR-stabilised block CG variants, other
 * Krylov methods, distributed plans, the C++ drop-in, the CLI, bench.py. */
#define SMFV_BLOCK_NEGATE 1 /* c = -C (exact) */
#define SMFV_BLOCK_MAX_K 128
SMFV_API int smfv_gram_workspace_bytes(int m, int Kx, int Ky, size_t *bytes);
SMFV_API int smfv_gram_host(int m, int Kx, int Ky, const double *h_X, int64_t ldx, const double *h_Y, int64_t ldy,
                            double *h_G, int64_t ldg);
SMFV_API int smfv_gram_f64(int m, int Kx, int Ky, const double *d_X, int64_t ldx, const double *d_Y, int64_t ldy,
                           double *d_G, int64_t ldg, double *d_workspace, void *stream);
SMFV_API int smfv_gram_set_tiling(int tiling);
SMFV_API int smfv_block_mul_f64(int m, int Kx, int Ky, int flags, const double *d_X, int64_t ldx, const double *d_C,
                                int64_t ldc, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, void *stream);
SMFV_API int smfv_small_solve_host(int K, int N, const double *h_G, int64_t ldg, const double *h_H, int64_t ldh,
                                   double *h_C, int64_t ldc);
SMFV_API int smfv_small_solve_f64(int K, int N, const double *d_G, int64_t ldg, const double *d_H, int64_t ldh,
                                  double *d_C, int64_t ldc, void *stream);

/* HBM streaming probe for the bench (not the SpMM path): d_dst = d_src,
 * `bytes` (multiple of 16, 16-B aligned pointers) by a 16-byte-per-lane
 * non-temporal copy kernel.  Read + write bytes / time = the measured
 * streaming ceiling quoted beside the 8 TB/s spec. */
SMFV_API int smfv_stream_copy(void *d_dst, const void *d_src, size_t bytes, void *stream);
/* (r6) Floor probe of the SpMM's 2:1 read:write mix (bench only).
 * unit_kib <= 0: a plain non-temporal stream, each 16 B written is the sum of
 * 32 B read (rbytes == 2 * wbytes).  unit_kib in 1..64: the same kind of
 * bytes through k_rows_ws's pipeline shape -- one 1024-lane block per CU,
 * loader waves staging units of unit_kib KiB of d_src into LDS by
 * non-temporal LDS-DMA (double-buffered), writer waves storing each unit's
 * share of wbytes from LDS; rbytes < 2 GiB, rbytes >= wbytes.  d_dst gets
 * no meaningful values. */
SMFV_API int smfv_stream_mix(void *d_dst, size_t wbytes, const void *d_src, size_t rbytes, int unit_kib,
                             void *stream);

/* Rank-local building blocks of the distributed variants (also usable on
 * their own).  Row block [row_begin, row_end) of Y (row-major, ldy):
 * what one rank of SC/...RowWise.cpp:36-50 computes.  n = rows of X (all
 * rank-local functions take it: it bounds every X access). */
SMFV_API int smfv_spmm_rowblock_f64(int row_begin, int row_end, int n, const int *d_row_ptr,
                                    const int *d_col_idx, const double *d_values,
                                    const double *d_X, int64_t ldx, int K,
                                    double *d_Yblock, int64_t ldy, void *stream);

/* Column panel [col_begin, col_end) of Y for all m rows, written as a
 * [m x (col_end-col_begin)] panel with leading dimension ldp: what one rank
 * of SC/...ColumnWise.cpp:34-48 computes. */
SMFV_API int smfv_spmm_colpanel_f64(int m, int n, int col_begin, int col_end, const int *d_row_ptr,
                                    const int *d_col_idx, const double *d_values,
                                    const double *d_X, int64_t ldx,
                                    double *d_panel, int64_t ldp, void *stream);

/* nnz range [nnz_begin, nnz_end) (SC/...NonZeroElement.cpp:56-67): partial
 * rows [row_first, row_last] written compactly to d_Ypart (row_last -
 * row_first + 1 rows, ldy).  row_first/row_last are returned by
 * smfv_nnz_range_rows (host, reads the host copy of row_ptr). */
SMFV_API int smfv_nnz_range_rows(int m, const int *h_row_ptr, int64_t nnz_begin, int64_t nnz_end,
                                 int *row_first, int *row_last);
SMFV_API int smfv_spmm_nnzrange_workspace_bytes(int nrows, int64_t nnz_count, int K, size_t *bytes);
SMFV_API int smfv_spmm_nnzrange_f64(int row_first, int row_last, int64_t nnz_begin, int64_t nnz_end,
                                    int n, const int *d_row_ptr, const int *d_col_idx,
                                    const double *d_values, const double *d_X, int64_t ldx, int K,
                                    double *d_Ypart, int64_t ldy,
                                    void *d_workspace, size_t workspace_bytes, void *stream);

/* Rebuild row-major Y from rank-major column panels (the rank-0 loop of
 * SC/...ColumnWise.cpp:109-126, on device): panels of p ranks laid out back
 * to back, rank r's panel is [m x kc_r] at offset sum_{q<r} m*kc_q. */
SMFV_API int smfv_panels_to_rowmajor_f64(int m, int K, int p, const double *d_panels,
                                         double *d_Y, int64_t ldy, void *stream);

/* Sum compact partial row blocks (one per rank, rank order) into Y, zeroing
 * rows no rank covers: the MPI_Reduce(SUM) of SC/...NonZeroElement.cpp:88
 * restricted to the rows each rank touched.  h_row_first/h_row_last are
 * host arrays of p entries; block r sits at d_blocks + offset_r where
 * offset_r = K * sum_{q<r} (row_last_q - row_first_q + 1) (empty ranks have
 * row_last = row_first - 1). */
SMFV_API int smfv_combine_row_blocks_f64(int m, int K, int p, const int *h_row_first,
                                         const int *h_row_last, const double *d_blocks,
                                         double *d_Y, int64_t ldy, void *stream);

/* Device-side areMatricesEqual (SC/utils.cpp:38-63): writes max |a-b| and
 * max |a-b|/max(|b|, tiny) over the m x K matrices into h_out[0..1]
 * (host memory; synchronises the stream). */
SMFV_API int smfv_compare_f64(int m, int K, const double *d_A, int64_t lda, const double *d_B,
                              int64_t ldb, double *h_out, void *stream);

/* ---- synthetic inputs generated on device (bench configs 4-5) ----------- */
/* X[i][k] = 1 + (splitmix64(seed ^ (i*K + k)) % 100): integers 1..100 like
 * SC/utils.cpp:203, but counter-based so any shard can be generated alone. */
SMFV_API int smfv_fill_x_hash_f64(int64_t n, int K, uint64_t seed, double *d_X, int64_t ldx,
                                  void *stream);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -------------------- */
typedef struct smfv_comm_s *smfv_comm_t;
#define SMFV_UNIQUE_ID_BYTES 128
SMFV_API int smfv_comm_unique_id(char out[SMFV_UNIQUE_ID_BYTES]);
SMFV_API int smfv_comm_init(smfv_comm_t *comm, int nranks, int rank,
                            const char id[SMFV_UNIQUE_ID_BYTES]);
SMFV_API int smfv_comm_destroy(smfv_comm_t comm);
SMFV_API int smfv_comm_rank(smfv_comm_t comm);
SMFV_API int smfv_comm_size(smfv_comm_t comm);
/* The number of ranks the RCCL communicator itself reports (ncclCommCount),
 * i.e. how many processes actually joined it -- not the size the caller
 * asked for.  (the reference's MPI_Comm_size(MPI_COMM_WORLD), SC/main.cpp:16) */
SMFV_API int smfv_comm_count(smfv_comm_t comm, int *nranks);
/* In-place broadcast of `bytes` device bytes from root's d_buf to every
 * rank's d_buf (ncclBroadcast over xGMI): the device-resident form of the
 * reference's input distribution (SC/main.cpp:106-143, 9x MPI_Bcast).
 * Collective, asynchronous on `stream`. */
SMFV_API int smfv_comm_bcast(smfv_comm_t comm, void *d_buf, size_t bytes, int root, void *stream);

/* Collective over `comm` (every rank calls it with the full A and X
 * resident on its device, as after SC/main.cpp:106-143):
 *   SMFV_ROWWISE    rank-local row block + gather (RowWise.cpp:85-87)
 *   SMFV_COLUMNWISE rank-local K panel + gather + device transpose (:82-84, :109-126)
 *   SMFV_NONZERO    rank-local nnz range + row-block reduce (NonZeroElement.cpp:88)
 * mode SMFV_TO_ROOT: the full Y lands on rank `root` only (reference
 * semantics, other ranks' d_Y untouched); SMFV_TO_ALL: every rank gets Y
 * (all-gather).  h_row_ptr is the host copy of row_ptr (NONZERO needs it to
 * find each rank's boundary rows).  Workspace: smfv_dist_workspace_bytes. */
/* Exchange plan of a distributed variant for p ranks (pure host; the same
 * function drives smfv_dist_spmm_f64).  For rank r:
 *   ROWWISE     first/last = its rows [first, last]            (RowWise.cpp:26-29)
 *   COLUMNWISE  first/last = its K columns [first, last]       (ColumnWise.cpp:25-28)
 *   NONZERO     first/last = the rows its nnz range touches    (NonZeroElement.cpp:24-39)
 * and offset/count (in doubles) = where its block sits in the exchange
 * buffer: Y itself for ROWWISE (offset = first*K), the rank-major panel
 * buffer for COLUMNWISE (offset = m*first), the compact row-block buffer for
 * NONZERO.  Empty ranks have last = first - 1 and count = 0.  Arrays hold p
 * entries; h_row_ptr is needed for NONZERO only. */
SMFV_API int smfv_dist_plan(int variant, int m, int64_t nnz, const int *h_row_ptr, int K, int p,
                            int *first, int *last, int64_t *offset, int64_t *count);

/* (r5) Distribution options: the high byte of a distributed plan's flags
 * (the low bits stay smfv_plan_create's SMFV_PLAN_* flags for the rank's
 * share), and the `dopts` of the *_opts host functions below.  0 = the
 * reference's decomposition.
 *   SMFV_DIST_BALANCED_ROWS  ROWWISE row blocks of equal WORK, 12 B per
 *        non-zero + 8K + 4 B per row (the block's CSR and Y bytes), instead
 *        of the reference's equal row counts (SC/...RowWise.cpp:26-29).  The
 *        result is bit-identical either way: each row is summed in CSR order
 *        by the one rank that owns it, and the Gatherv / all-gatherv exchange
 *        takes any block sizes.  Opt-in: measured on the irregular cop20k_A
 *        stand-in at p = 8 it cuts the slowest rank's kernel 12.1 -> 11.5 us
 *        but makes the Y blocks unequal (the largest 3.9 -> 5.6 MB), so the
 *        exchange, which dominates the step, loses the single ncclAllGather
 *        and moves more bytes per link.
 *   SMFV_DIST_CHUNKS(c)  ROWWISE, c = 2..7: the rank's block is cut into c
 *        row chunks of equal work, each a row-block plan of its own; chunk
 *        j's exchange is issued on the plan's exchange stream as soon as
 *        chunk j is computed, while chunk j + 1 computes (the exchange of
 *        one problem overlapped with its own compute).  A chunk's exchange
 *        is point to point: ncclSend of the chunk to every peer and ncclRecv
 *        of theirs (TO_ALL, an all-gatherv over the full xGMI mesh) or to the
 *        root (TO_ROOT, the Gatherv).  0 / 1: one block, one exchange.
 *        EXPERIMENTAL: the schedule is pinned over gloo (2 / 3 / 8 ranks) and
 *        at one rank on the GPU; its RCCL point-to-point groups have not yet
 *        moved data between two GPUs, so bench.py defaults to --chunks 1.
 * Row-partitioned plans (A not replicated) always use the reference rows. */
#define SMFV_DIST_BALANCED_ROWS (1 << 24)
#define SMFV_DIST_CHUNKS(c) (((c) & 7) << 25)
#define SMFV_DIST_CHUNKS_OF(f) (((f) >> 25) & 7)
#define SMFV_DIST_OPTS ((int)0xFF000000u) /* (r6) no signed shift into the sign bit */
/* smfv_dist_plan under distribution options (h_row_ptr needed for
 * work-balanced ROWWISE blocks; NULL falls back to the reference rows).
 * smfv_dist_plan(...) = smfv_dist_plan_opts(..., 0). */
SMFV_API int smfv_dist_plan_opts(int variant, int dopts, int m, int64_t nnz, const int *h_row_ptr, int K, int p,
                                 int *first, int *last, int64_t *offset, int64_t *count);
/* ROWWISE under SMFV_DIST_CHUNKS(c): rank `rank`'s chunk boundaries,
 * chunk j = rows [bounds[j], bounds[j + 1]); bounds holds >= 8 entries,
 * *nchunks receives c (1 when unchunked: bounds = [first, last + 1]). */
SMFV_API int smfv_dist_chunk_rows(int variant, int dopts, int m, int64_t nnz, const int *h_row_ptr, int K, int p,
                                  int rank, int *bounds, int *nchunks);

typedef enum smfv_dist_mode { SMFV_TO_ROOT = 0, SMFV_TO_ALL = 1 } smfv_dist_mode;
SMFV_API int smfv_dist_workspace_bytes(smfv_comm_t comm, int variant, int m, int64_t nnz,
                                       const int *h_row_ptr, int K, size_t *bytes);
SMFV_API int smfv_dist_spmm_f64(smfv_comm_t comm, int variant, int mode, int root, int m, int n,
                                int64_t nnz, const int *h_row_ptr, const int *d_row_ptr,
                                const int *d_col_idx, const double *d_values, const double *d_X,
                                int K, double *d_Y, void *d_workspace, size_t workspace_bytes,
                                void *stream);

/* Row-partitioned ROWWISE (bench config 5: the matrix does not fit, or is
 * not wanted, on every rank).  Unlike smfv_dist_spmm_f64, A is NOT
 * replicated: rank r passes only its rows [first, last] of the RowWise
 * partition (SC/...RowWise.cpp:26-29; smfv_dist_plan) as a local CSR
 * (row_ptr 0-based, column ids global), X (n x K, row-major) replicated.
 * Rank r computes its block in place at d_Y + first*K (d_Y is m x K on
 * every rank), then the RowWise exchange: SMFV_TO_ALL all-gathers (one
 * ncclAllGather when the blocks are equal, else all-gatherv),
 * SMFV_TO_ROOT gathers to root (SC/...RowWise.cpp:85-87).  Collective. */
SMFV_API int smfv_dist_rowpart_spmm_f64(smfv_comm_t comm, int mode, int root, int m, int n,
                                        const int *d_row_ptr_local, const int *d_col_idx_local,
                                        const double *d_values_local, const double *d_X, int K,
                                        double *d_Y, void *stream);

/* The exchange step as a list of operations (pure host; the schedule
 * smfv_dist_spmm_f64 and the distributed plans execute with RCCL, exposed so
 * it can be replayed over another transport in tests).  For rank `rank` of
 * p: op i is kinds[i] (SMFV_EX_*) with peer, offset and count (doubles,
 * into the exchange buffer of smfv_dist_plan); ops run in order, inside
 * one group.  Arrays hold >= 2p entries; *nops receives the count. */
#define SMFV_EX_ALLGATHER 1 /* ncclAllGather(buf + offset, buf + offset - rank * count, count): equal
                              back-to-back blocks, rank r's at offset - (rank - r) * count */
#define SMFV_EX_BCAST 2     /* ncclBroadcast(buf + offset, count, root = peer): one block of an all-gatherv */
#define SMFV_EX_SEND 3      /* ncclSend(buf + offset, count, to peer): own block to the root */
#define SMFV_EX_RECV 4      /* ncclRecv(buf + offset, count, from peer): a rank's block at the root */
SMFV_API int smfv_dist_exchange_ops(int variant, int mode, int root, int m, int64_t nnz,
                                    const int *h_row_ptr, int K, int p, int rank, int *kinds, int *peers,
                                    int64_t *offsets, int64_t *counts, int *nops);
/* (r5) The same under distribution options: the ops of chunk `chunk` (0 when
 * unchunked); a chunked plan runs chunk j's ops after chunk j's compute. */
SMFV_API int smfv_dist_exchange_ops_opts(int variant, int dopts, int mode, int root, int m, int64_t nnz,
                                         const int *h_row_ptr, int K, int p, int rank, int chunk, int *kinds,
                                         int *peers, int64_t *offsets, int64_t *counts, int *nops);
/* Runs an exchange schedule (ops as smfv_dist_exchange_ops returns them, or
 * any list of the same form) on `comm` over the device buffer d_buf:
 * ncclAllGather alone, else one ncclGroupStart / ncclGroupEnd around the
 * broadcasts / sends / receives.  A failing RCCL call closes the group
 * before the error returns, so the communicator's next call starts clean.
 * Collective; asynchronous on `stream`. */
SMFV_API int smfv_comm_exchange_f64(smfv_comm_t comm, const int *kinds, const int *peers, const int64_t *offsets,
                                    const int64_t *counts, int nops, double *d_buf, void *stream);
/* Test hook: the nth exchange operation run from now on (any communicator,
 * any plan) fails as an RCCL error would, inside its open group; 0 = off. */
SMFV_API void smfv_test_fail_exchange(int nth);

/* ---- distributed plans: the rank-local part analysed once --------------
 * A distributed plan holds this rank's share of a variant (RowWise row
 * block, ColumnWise K-column window, NonZeroElement nnz range) as a
 * single-device plan -- so the rank-local compute runs the tiled kernel
 * where it pays, as smfv_plan_* does -- plus the exchange buffers and the
 * exchange schedule.  h_col_idx may be NULL (no tiling).  Values contract as
 * for smfv_plan_t (bind after a change).  execute = execute_local +
 * exchange on the same stream; the two halves are exposed separately for
 * timing.  mode / root as smfv_dist_spmm_f64; d_Y is m x K, row-major.
 * Collective: every rank creates and executes its plan. */
typedef struct smfv_dist_plan_s *smfv_dist_plan_t;
SMFV_API int smfv_dist_plan_create(smfv_dist_plan_t *plan, smfv_comm_t comm, int variant, int mode, int root,
                                   int m, int n, int64_t nnz, const int *h_row_ptr, const int *h_col_idx, int K,
                                   int flags);
/* Row-partitioned ROWWISE (A not replicated, as smfv_dist_rowpart_spmm_f64):
 * the rank's local CSR rows of the RowWise partition of an m-row matrix. */
SMFV_API int smfv_dist_plan_create_rowpart(smfv_dist_plan_t *plan, smfv_comm_t comm, int mode, int root, int m,
                                           int n, const int *h_row_ptr_local, const int *h_col_idx_local, int K,
                                           int flags);
/* The plan of rank `rank` of `p` with no communicator: the rank-local share
 * exactly as a rank of smfv_dist_plan_create computes it (same partition,
 * same single-device plan), execute_local only -- exchange and execute
 * return SMFV_ERR_COMM when the schedule has operations.  Lets one device
 * run every rank of a p-rank decomposition (tests, replays). */
SMFV_API int smfv_dist_plan_create_rank(smfv_dist_plan_t *plan, int p, int rank, int variant, int mode, int root,
                                        int m, int n, int64_t nnz, const int *h_row_ptr, const int *h_col_idx, int K,
                                        int flags);
/* The plan's exchange buffer (device; COLUMNWISE rank-major panels, NONZERO
 * compact row blocks, at smfv_dist_plan's offset / count) and its size in
 * doubles; NULL / 0 for ROWWISE, whose exchange runs in Y. */
SMFV_API int smfv_dist_plan_exchange_buffer(smfv_dist_plan_t plan, double **d_buf, int64_t *doubles);
/* (r5) The partition the plan was created with (p entries each, as
 * smfv_dist_plan_opts returns them) and its p, rank and chunks per rank. */
SMFV_API int smfv_dist_plan_partition(smfv_dist_plan_t plan, int *first, int *last, int64_t *offset,
                                      int64_t *count);
SMFV_API int smfv_dist_plan_shape(smfv_dist_plan_t plan, int *p, int *rank, int *chunks);
SMFV_API int smfv_dist_plan_bind_values(smfv_dist_plan_t plan, const double *d_values, void *stream);
SMFV_API int smfv_dist_plan_execute(smfv_dist_plan_t plan, const int *d_row_ptr, const int *d_col_idx,
                                    const double *d_values, const double *d_X, double *d_Y, void *stream);
SMFV_API int smfv_dist_plan_execute_local(smfv_dist_plan_t plan, const int *d_row_ptr, const int *d_col_idx,
                                          const double *d_values, const double *d_X, double *d_Y, void *stream);
SMFV_API int smfv_dist_plan_exchange(smfv_dist_plan_t plan, double *d_Y, void *stream);
/* the rank-local plan's smfv_plan_stats */
SMFV_API int smfv_dist_plan_stats(smfv_dist_plan_t plan, double out[SMFV_PLAN_STATS]);
SMFV_API int smfv_dist_plan_destroy(smfv_dist_plan_t plan);

/* ---- vendor-library comparator (not on the product path) ---------------
 * Y = A * X by rocSPARSE's generic SpMM (CSR int32 / f64, row-major X and
 * Y), the analogue of the reference's PETSc MatMatMult comparison block
 * (SC/main.cpp:289-402).  create binds the operands, sizes and allocates the
 * rocSPARSE buffer and runs its preprocess stage; execute runs the compute
 * stage on the stream given at creation.  alg: 0 rocSPARSE default, 1 CSR
 * row split, 2 CSR merge path.  rocSPARSE's summation order is its own: its
 * result matches the reference within tolerance, not bit for bit. */
typedef struct smfv_vendor_s *smfv_vendor_t;
SMFV_API int smfv_vendor_spmm_create(smfv_vendor_t *handle, int alg, int m, int n, int64_t nnz,
                                     const int *d_row_ptr, const int *d_col_idx, const double *d_values,
                                     const double *d_X, int64_t ldx, int K, double *d_Y, int64_t ldy,
                                     void *stream);
SMFV_API int smfv_vendor_spmm_execute(smfv_vendor_t handle);
SMFV_API int smfv_vendor_spmm_destroy(smfv_vendor_t handle);

#ifdef __cplusplus
}
#endif

#endif /* SMFV_H */
