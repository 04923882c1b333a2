"""Parity of the HIP kernels (through the C ABI) with the reference.

Bit-exact: SEQUENTIAL / ROWWISE / COLUMNWISE against the reference's own
outputs (golden fixtures) and against the oracle on larger inputs.
NONZERO (merge-path; on one device with X-row re-use the tiled row kernel,
bit-identical): deterministic, within 1e-12 of the sequential result
relative to sum|a||x| (tolerance written here; the north star allows 1e-6
relative, the reference's own check is 1e-6 absolute, SC/utils.cpp:55).
"""
import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden
from oracle import oracle

import sparsematrixmultiplicationmpi_amd as smfv
from sparsematrixmultiplicationmpi_amd import engine as S

pytestmark = pytest.mark.gpu
NNZ_TOL = 1e-12
CASES = sorted(golden_cases())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mat(rp, ci, va, m, n):
    return smfv.SparseMatrix(np.asarray(va, np.float64), np.asarray(ci, np.int32),
                             np.asarray(rp, np.int32), int(m), int(n))


def rel_err(Y, Yref, absY):
    return oracle.max_rel_err(Y, Yref, absY)


def run(variant, A, X, gpu, ldx_pad=0, ldy_pad=0):
    dA = smfv.DeviceCSR(A, gpu)
    K = X.shape[1]
    Xb = torch.zeros((A.numCols, K + ldx_pad), dtype=torch.float64, device=gpu)
    Xd = Xb[:, :K]
    Xd.copy_(torch.from_numpy(np.ascontiguousarray(X)))
    Yb = torch.full((A.numRows, K + ldy_pad), np.nan, dtype=torch.float64, device=gpu)
    Yd = Yb[:, :K]
    smfv.SpmmPlan(variant, dA, K).run(Xd, Yd)
    torch.cuda.synchronize()
    if ldy_pad:  # padding must be untouched
        assert torch.isnan(Yb[:, K:]).all()
    return Yd.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("variant", list(smfv.Variant))
def test_golden(gpu, name, variant):
    g = load_golden(name)
    A = mat(g["row_ptr"], g["col_idx"], g["values"], g["m"], g["n"])
    Y = run(variant, A, g["X"], gpu)
    if variant == smfv.Variant.NONZERO:
        absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(g["X"]))
        assert rel_err(Y, g["Y_seq"], absY) <= NNZ_TOL
    else:
        assert np.array_equal(bits(Y), bits(g["Y_seq"]))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 7, 8, 15, 16, 31, 32, 33, 64, 100, 127, 128, 129, 200])
def test_k_sweep_fem(gpu, K):
    A = smfv.gen_fem27(3000, 14, 14, 0.8, K)
    X = np.random.default_rng(K).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    for v in (smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE):
        assert np.array_equal(bits(run(v, A, X, gpu)), bits(Yref)), v
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    assert rel_err(run(smfv.Variant.NONZERO, A, X, gpu), Yref, absY) <= NNZ_TOL


@pytest.mark.parametrize("pads", [(1, 0), (0, 1), (3, 5)])
def test_unaligned_leading_dims(gpu, pads):
    A = smfv.gen_fem27(2000, 12, 12, 0.8, 9)
    X = np.random.default_rng(9).uniform(-1, 1, (A.numCols, 32))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    for v in smfv.Variant:
        Y = run(v, A, X, gpu, *pads)
        if v == smfv.Variant.NONZERO:
            assert np.max(np.abs(Y - Yref)) <= 1e-9
        else:
            assert np.array_equal(bits(Y), bits(Yref)), v


def test_powerlaw_long_rows(gpu):
    """Rows up to 4096 nnz (merge-path splits them across teams)."""
    A = smfv.gen_random_rows(60000, 50000, 16, 2.0, 4096, 3)
    assert np.diff(A.rowPtr).max() >= 1000
    X = np.random.default_rng(3).uniform(-1, 1, (A.numCols, 32))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    assert np.array_equal(bits(run(smfv.Variant.ROWWISE, A, X, gpu)), bits(Yref))
    Yz = run(smfv.Variant.NONZERO, A, X, gpu)
    assert rel_err(Yz, Yref, absY) <= NNZ_TOL
    # deterministic: same bits on a second run
    assert np.array_equal(bits(run(smfv.Variant.NONZERO, A, X, gpu)), bits(Yz))


def test_single_huge_row_and_empty_rows(gpu):
    m, n = 50, 40000
    lens = np.zeros(m, np.int64)
    lens[7] = 30000
    lens[[0, 1, 20]] = [3, 1, 5]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(5)
    ci = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
    A = mat(rp, ci, rng.uniform(-1, 1, rp[-1]), m, n)
    X = rng.uniform(-1, 1, (n, 16))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    for v in smfv.Variant:
        Y = run(v, A, X, gpu)
        assert np.all(Y[lens == 0] == 0.0)
        if v == smfv.Variant.NONZERO:
            assert rel_err(Y, Yref, absY) <= NNZ_TOL
        else:
            assert np.array_equal(bits(Y), bits(Yref)), v


def test_degenerate_sizes(gpu):
    # m = 0
    A = mat([0], [], [], 0, 5)
    for v in smfv.Variant:
        assert run(v, A, np.ones((5, 4)), gpu).shape == (0, 4)
    # nnz = 0: Y must be all zeros
    A = mat([0, 0, 0, 0], [], [], 3, 4)
    for v in smfv.Variant:
        assert np.all(run(v, A, np.ones((4, 3)), gpu) == 0.0)
    # no columns at all (n = 0, X has no rows) at K = 1 and 32: Y is zeros
    A = mat([0, 0, 0], [], [], 2, 0)
    for K in (1, 32):
        for v in smfv.Variant:
            assert np.all(run(v, A, np.ones((0, K)), gpu) == 0.0), (v, K)
    # K = 0
    A = smfv.gen_fem27(100, 5, 5, 0.8, 1)
    for v in smfv.Variant:
        assert run(v, A, np.ones((100, 0)), gpu).shape == (100, 0)


def test_cop20k_surrogate_full_size(gpu):
    """BASELINE config 2/3 at full size against the oracle, bit for bit."""
    A = smfv.cop20k_surrogate()
    assert A.numRows == smfv.COP20K_M and abs(A.nnz - smfv.COP20K_NNZ) < 100
    for K in (32, 128):
        X = smfv.generateLargeFatVector(A.numCols, K)
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
        Y = run(smfv.Variant.ROWWISE, A, X, gpu)
        assert np.array_equal(bits(Y), bits(Yref)), K
        # the reference's own acceptance check (absolute 1e-6, SC/utils.cpp:55)
        assert smfv.areMatricesEqual(run(smfv.Variant.NONZERO, A, X, gpu), Yref, 1e-6)


def test_cop20k_irregular_surrogate_full_size(gpu):
    """The second, unstructured cop20k_A stand-in (same m and nnz; k-NN graph
    of clustered 3-D points, row degrees 4..85) at full size: the default
    plan tiles it and every variant's one-device result is bit-identical to
    the reference order at K = 32 (NONZERO on the merge path within 1e-12)."""
    A = smfv.inputs.cop20k_irregular_surrogate()
    d = np.diff(A.rowPtr)
    assert A.numRows == smfv.COP20K_M and abs(A.nnz - smfv.COP20K_NNZ) < 100 and d.min() <= 5 and d.max() >= 70
    K = 32
    X = smfv.generateLargeFatVector(A.numCols, K)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for v in smfv.Variant:
        plan = smfv.SpmmPlan(v, dA, K)
        assert plan.stats()["tiled"], v
        Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dX, Y)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref)), v
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    smfv.SpmmPlan(smfv.Variant.NONZERO, dA, K, tiles="off").run(dX, Y)
    torch.cuda.synchronize()
    assert rel_err(Y.cpu().numpy(), Yref, absY) <= NNZ_TOL


def test_cop20k_surrogate_full_size_k1(gpu):
    """Config 1's GPU line (K = 1, k_spmv_stream) at full size on the cop20k
    surrogate: bit-identical to the reference order for every variant but
    NONZERO (merge path, within 1e-12 x sum|a||x|)."""
    A = smfv.cop20k_surrogate()
    X = smfv.generateLargeFatVector(A.numCols, 1)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    for v in smfv.Variant:
        Y = run(v, A, X, gpu)
        if v == smfv.Variant.NONZERO:
            assert rel_err(Y, Yref, absY) <= NNZ_TOL
        else:
            assert np.array_equal(bits(Y), bits(Yref)), v


def test_nonzero_one_device_plan_choice(gpu):
    """NONZERO on one device: on a pattern with X-row re-use the plan takes
    the tiled row kernel and equals the sequential sum bit for bit -- what the
    reference's NonZeroElement computes with one rank (its single nnz range
    sums every row in CSR order, SC/...NonZeroElement.cpp:56-67); tiles="off"
    keeps the nnz-balanced merge path (within 1e-12 of sum|a||x|, deterministic);
    a re-use-free power-law pattern stays on the merge path."""
    A = smfv.cop20k_surrogate()
    K = 32
    X = smfv.generateLargeFatVector(A.numCols, K)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    tiled = smfv.SpmmPlan(smfv.Variant.NONZERO, dA, K)
    merge = smfv.SpmmPlan(smfv.Variant.NONZERO, dA, K, tiles="off")
    assert tiled.stats()["tiled"] and not merge.stats()["tiled"]
    outs = []
    for plan in (tiled, merge, merge):
        Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dX, Y)
        torch.cuda.synchronize()
        outs.append(Y.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(Yref))
    assert rel_err(outs[1], Yref, absY) <= NNZ_TOL and np.array_equal(bits(outs[1]), bits(outs[2]))
    B = smfv.gen_random_rows(60000, 50000, 16, 2.0, 4096, 3)
    assert not smfv.SpmmPlan(smfv.Variant.NONZERO, smfv.DeviceCSR(B, gpu), K).stats()["tiled"]


def test_rank_local_building_blocks(gpu):
    """rowblock / colpanel / nnzrange + panels_to_rowmajor + combine reproduce
    the reference's per-rank pieces for p = 1, 2, 3, 8."""
    A = smfv.gen_random_rows(5000, 4000, 12, 2.0, 600, 17)
    K = 8
    X = np.random.default_rng(17).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    absY = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for p in (1, 2, 3, 8):
        # RowWise blocks
        Y = torch.zeros((A.numRows, K), dtype=torch.float64, device=gpu)
        for r in range(p):
            s, e = oracle.partition_rows(A.numRows, p, r)
            S.spmm_rowblock(dA, s, e, dX, Y[s:e])
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))
        # ColumnWise panels -> rank-major buffer -> device rebuild
        panels = torch.zeros(A.numRows * K, dtype=torch.float64, device=gpu)
        for r in range(p):
            c0, c1 = oracle.partition_cols(K, p, r)
            if c1 > c0:
                S.spmm_colpanel(dA, c0, c1, dX, panels[A.numRows * c0: A.numRows * c1].view(A.numRows, c1 - c0))
        Y2 = torch.empty((A.numRows, K), dtype=torch.float64, device=gpu)
        smfv._lib.call("smfv_panels_to_rowmajor_f64", A.numRows, K, p, panels.data_ptr(), Y2.data_ptr(), K,
                       S.stream_handle())
        assert np.array_equal(bits(Y2.cpu().numpy()), bits(Yref))
        # NonZeroElement ranges -> compact blocks -> combine
        rfs, rls, blocks = [], [], []
        for r in range(p):
            s, e = oracle.partition_nnz(A.nnz, p, r)
            rf, rl, Yp = S.spmm_nnzrange(dA, s, e, dX)
            rfs.append(rf), rls.append(rl), blocks.append(Yp.reshape(-1))
        buf = torch.cat(blocks) if blocks else torch.zeros(1, dtype=torch.float64, device=gpu)
        Y3 = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        import ctypes
        rfa = (ctypes.c_int * p)(*rfs)
        rla = (ctypes.c_int * p)(*rls)
        smfv._lib.call("smfv_combine_row_blocks_f64", A.numRows, K, p, rfa, rla, buf.data_ptr(), Y3.data_ptr(),
                       K, S.stream_handle())
        torch.cuda.synchronize()
        assert rel_err(Y3.cpu().numpy(), Yref, absY) <= NNZ_TOL, p


def test_compare_and_fill(gpu):
    a = torch.randn(300, 7, dtype=torch.float64, device=gpu)
    b = a.clone()
    b[17, 3] += 0.5
    mabs, mrel = smfv.compare(a, b)
    assert mabs == pytest.approx(0.5)
    X = torch.empty((1000, 32), dtype=torch.float64, device=gpu)
    smfv.fill_x_hash(X, 43)
    Xh = X.cpu().numpy()
    assert Xh.min() >= 1 and Xh.max() <= 100 and np.all(Xh == np.round(Xh))
    X2 = torch.empty((1000, 32), dtype=torch.float64, device=gpu)
    smfv.fill_x_hash(X2, 43)
    assert torch.equal(X, X2)


def test_mix_floor_probe_moves_the_bytes(gpu):
    """(r6) The 2:1 floor probes bench.py reports (roofline.mix_matched_copy)
    really move their bytes: plain mode writes the sum of each 32-B pair it
    reads; the LDS-DMA mode writes, for unit u of ru bytes, the bytes its
    loaders staged (dst[u wu + i] = src[u ru + i mod ru] wherever that
    source byte exists).  Sizes like the headline's ratio, small."""
    from sparsematrixmultiplicationmpi_amd._lib import call
    st = torch.cuda.current_stream().cuda_stream
    w = 3 * 1000 * 1024 + 48  # not a multiple of the unit: ragged last unit
    src = torch.randn(2 * w // 8, dtype=torch.float64, device=gpu)
    dst = torch.zeros(w // 8, dtype=torch.float64, device=gpu)
    call("smfv_stream_mix", dst.data_ptr(), w, src.data_ptr(), 2 * w, 0, st)
    torch.cuda.synchronize()
    pairs = src.view(-1, 2, 2)  # 16-B pieces of two doubles
    assert torch.equal(dst.view(-1, 2), pairs[:, 0, :] + pairs[:, 1, :])
    for unit_kib in (32, 64):
        r = 2 * w - 16 * 37  # reads >= writes, ragged
        dst.zero_()
        call("smfv_stream_mix", dst.data_ptr(), w, src.data_ptr(), r, unit_kib, st)
        torch.cuda.synchronize()
        ru = unit_kib * 1024
        nunits = (r + ru - 1) // ru
        wu = ((w + nunits - 1) // nunits + 15) // 16 * 16
        sb = src.view(torch.uint8).cpu().numpy()
        db = dst.view(torch.uint8).cpu().numpy()
        for u in range(nunits):
            i = np.arange(u * wu, min((u + 1) * wu, w))
            srci = u * ru + (i - u * wu) % ru
            ok = srci < r
            assert np.array_equal(db[i[ok]], sb[srci[ok]]), (unit_kib, u)
    with pytest.raises(RuntimeError):  # plain mode reads exactly twice what it writes
        call("smfv_stream_mix", dst.data_ptr(), w, src.data_ptr(), w, 0, st)


def test_reference_api_functions(gpu):
    """The reference's four entry points (host arrays in/out), single process."""
    g = load_golden("fem1k_k32")
    A = mat(g["row_ptr"], g["col_idx"], g["values"], g["m"], g["n"])
    K = g["X"].shape[1]
    for fn in (smfv.sparseMatrixFatVectorMultiply, smfv.sparseMatrixFatVectorMultiplyRowWise,
               smfv.sparseMatrixFatVectorMultiplyColumnWise):
        assert np.array_equal(bits(fn(A, g["X"], K)), bits(g["Y_seq"]))
    assert smfv.areMatricesEqual(smfv.sparseMatrixFatVectorMultiplyNonZeroElement(A, g["X"], K), g["Y_seq"], 1e-6)


def test_errors_are_loud(gpu):
    A = smfv.gen_fem27(100, 5, 5, 0.8, 1)
    dA = smfv.DeviceCSR(A, gpu)
    X = torch.ones((100, 4), dtype=torch.float64, device=gpu)
    Y = torch.empty((100, 4), dtype=torch.float64, device=gpu)
    with pytest.raises(smfv.SmfvError):
        smfv._lib.call("smfv_spmm_csr_f64", 9, 100, 100, A.nnz, *dA.ptrs(), X.data_ptr(), 4, 4, Y.data_ptr(), 4,
                       None, 0, None)
    with pytest.raises(smfv.SmfvError):  # NONZERO without workspace
        smfv._lib.call("smfv_spmm_csr_f64", 3, 100, 100, A.nnz, *dA.ptrs(), X.data_ptr(), 4, 4, Y.data_ptr(), 4,
                       None, 0, None)
    with pytest.raises(smfv.SmfvError):  # ldx < K
        smfv._lib.call("smfv_spmm_csr_f64", 1, 100, 100, A.nnz, *dA.ptrs(), X.data_ptr(), 2, 4, Y.data_ptr(), 4,
                       None, 0, None)


def test_dist_single_rank(gpu):
    """The RCCL path with one rank (the box has one GPU): plan + exchange code
    runs end to end, every variant and mode."""
    from sparsematrixmultiplicationmpi_amd import dist as D
    comm = D.Communicator(0, 1, D.Communicator.new_unique_id())
    A = smfv.gen_random_rows(3000, 3000, 10, 2.0, 300, 23)
    K = 16
    X = np.random.default_rng(23).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for v in smfv.Variant:
        for to_all in (False, True):
            Y = D.dist_spmm(comm, v, dA, dX, to_all=to_all)
            torch.cuda.synchronize()
            Yh = Y.cpu().numpy()
            if v == smfv.Variant.NONZERO:
                assert np.max(np.abs(Yh - Yref)) <= 1e-10
            else:
                assert np.array_equal(bits(Yh), bits(Yref)), (v, to_all)
    comm.close()


@pytest.mark.parametrize("K", [32, 64, 128, 96])
def test_tiled_plan_bitwise(gpu, K):
    """The LDS-tiled row kernel (plan with tiles) is bit-identical to the
    reference order for every tiling mode, including tiles that fall back to
    direct gathers (rows wider than the LDS union)."""
    rng = np.random.default_rng(K)
    for A in (smfv.gen_fem27(5000, 12, 12, 0.83, K),
              smfv.gen_random_rows(6000, 5000, 16, 2.0, 1500, K)):  # rows up to 1500 wide
        X = rng.uniform(-1, 1, (A.numCols, K))
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
        dA = smfv.DeviceCSR(A, gpu)
        dX = torch.from_numpy(X).to(gpu)
        for mode in ("force", "auto", "off"):
            for v in (smfv.Variant.SEQUENTIAL, smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE):
                plan = smfv.SpmmPlan(v, dA, K, tiles=mode)
                Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
                plan.run(dX, Y)
                torch.cuda.synchronize()
                assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref)), (mode, v, plan.stats())
                if mode == "force":
                    assert plan.stats()["tiled"]


@pytest.mark.parametrize("K", [4, 8, 16])
def test_tiled_narrow_window_bitwise(gpu, K):
    """(r4) K = 4 / 8 / 16 -- a ColumnWise rank's K/p panel (SC/...ColumnWise.cpp:34-48)
    -- on the tiled kernel: the column window [f, f + K) of a 32-wide X (X + f,
    the full row stride) into a Y panel whose padded stride must stay
    untouched (NaN): the kernel stages and stores only the window's columns.
    Bit-identical to the reference's sequential sum, including direct rows
    (rows wider than the LDS union, k_rows_list)."""
    rng = np.random.default_rng(100 + K)
    for A in (smfv.gen_fem27(5000, 12, 12, 0.83, K),
              smfv.gen_random_rows(6000, 5000, 16, 2.0, 1500, K)):  # rows up to 1500 wide
        X = rng.uniform(-1, 1, (A.numCols, 32))
        dA = smfv.DeviceCSR(A, gpu)
        dXf = torch.from_numpy(X).to(gpu)
        for f in (0, 32 - K):
            Xw = np.ascontiguousarray(X[:, f:f + K])
            Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, Xw)
            for mode in ("force", "auto"):
                for v in (smfv.Variant.SEQUENTIAL, smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE):
                    plan = smfv.SpmmPlan(v, dA, K, tiles=mode)
                    Yb = torch.full((A.numRows, K + 2), np.nan, dtype=torch.float64, device=gpu)
                    plan.run(dXf[:, f:f + K], Yb[:, :K])
                    torch.cuda.synchronize()
                    assert np.array_equal(bits(Yb[:, :K].cpu().numpy()), bits(Yref)), (f, mode, v, plan.stats())
                    assert torch.isnan(Yb[:, K:]).all()
                    if mode == "force":
                        assert plan.stats()["tiled"]


@pytest.mark.parametrize("tk", ["ws1", "ws2", "ws3", "fma"])
def test_tiled_narrow_window_instances(gpu, tk):
    """(r4) Every NARROW instance of k_rows_ws (geometries 1 / 2 / 3, and the
    FMA opt-in within 1e-12 x sum|a||x|) on an 8-column window of a 32-wide
    X, on a pattern large enough for several units per block."""
    K, f = 8, 16
    A = smfv.gen_fem27(40000, 30, 30, 0.83, 5)
    X = np.random.default_rng(5).uniform(-1, 1, (A.numCols, 32))
    Xw = np.ascontiguousarray(X[:, f:f + K])
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, Xw)
    dA = smfv.DeviceCSR(A, gpu)
    dXf = torch.from_numpy(X).to(gpu)
    plan = (smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", fma=True) if tk == "fma"
            else smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", tiled_kernel=tk))
    st = plan.stats()
    assert st["tiled"] and (tk == "fma" or st["ws_geom"] == int(tk[-1])), st
    Yb = torch.full((A.numRows, K + 2), np.nan, dtype=torch.float64, device=gpu)
    plan.run(dXf[:, f:f + K], Yb[:, :K])
    torch.cuda.synchronize()
    Y = Yb[:, :K].cpu().numpy()
    if tk == "fma":
        scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(Xw))
        assert np.all(np.abs(Y - Yref) <= 1e-12 * scale + 1e-300)
    else:
        assert np.array_equal(bits(Y), bits(Yref)), st
    assert torch.isnan(Yb[:, K:]).all()


def test_tiled_plan_stats_cop20k(gpu):
    A = smfv.cop20k_surrogate()
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(A, gpu), 32)
    st = plan.stats()
    assert st["reuse"] > 1.9 and st["direct_rows"] == 0
    assert st["est_reuse"] >= 3.0 and st["tiled"]  # sampled estimate (128 tiles in the full pattern)
    assert st["analysis_ms"] < 2000.0  # ~0.1 s on the box; a generous bound, not a benchmark


def test_untiled_pattern_rejected_by_sample(gpu):
    """A pattern without X-row re-use (uniform random columns) is rejected by
    the tile sample before any full-pattern pass (parts, footprints): the
    analysis stays a small fraction of what the r2 order cost (6.3 s on
    pow10m), so an untiled first call never waits on it."""
    m = 2_000_000
    A = smfv.gen_random_rows(m, m, 16.0, 0.0, 16, 11)
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(A, gpu), 32)
    st = plan.stats()
    assert not st["tiled"] and st["est_reuse"] < 1.5, st
    assert st["analysis_ms"] < 1500.0, st


def test_dist_rowpart_single_rank(gpu):
    """Row-partitioned ROWWISE (bench config 5's path) on one rank: the local
    CSR is the whole matrix, the exchange is a no-op; bit-identical."""
    from sparsematrixmultiplicationmpi_amd import dist as D
    comm = D.Communicator(0, 1, D.Communicator.new_unique_id())
    m = 5000
    A = smfv.gen_random_rows(m, m, 16.0, 0.0, 16, 42)
    K = 32
    X = np.random.default_rng(5).uniform(-1, 1, (m, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    Y = torch.full((m, K), np.nan, dtype=torch.float64, device=gpu)
    D.dist_rowpart_spmm(comm, m, dA, torch.from_numpy(X).to(gpu), Y, to_all=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))
    comm.close()


@pytest.mark.parametrize("name", ["sym5.mtx", "pat4x6.mtx", "empty7x5.mtx"])
@pytest.mark.parametrize("K", [32, 64])
def test_tiled_plan_tiny(gpu, name, K):
    """Forced tiles on matrices with fewer tiles than XCDs (one tile, empty
    rows, a duplicate entry): every row is still computed, bit-identical."""
    import os
    A = smfv.readMatrixMarketFile(os.path.join(os.path.dirname(__file__), "golden", name))
    X = np.random.default_rng(K).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force")
    assert plan.stats()["tiled"]
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(torch.from_numpy(X).to(gpu), Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))


@pytest.mark.parametrize("K", [32, 128])
def test_tiled_plan_every_row_length(gpu, K):
    """Row lengths 0..40 (every residue mod 8: rows ending on a half batch of
    4 entries, on a whole batch of 8, or both) in forced tiles, columns from a
    local window so rows share X rows; bit-identical to the reference order."""
    rng = np.random.default_rng(7 + K)
    m = n = 3000
    lens = np.arange(m) % 41
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(np.arange(max(0, i - 60), min(n, i + 60)), L, replace=False))
                         for i, L in enumerate(lens)]).astype(np.int32)
    A = smfv.SparseMatrix(values=rng.uniform(-1, 1, ci.size), colIndices=ci, rowPtr=rp, numRows=m, numCols=n)
    X = rng.uniform(-1, 1, (n, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(A, gpu), K, tiles="force")
    assert plan.stats()["tiled"]
    Y = torch.full((m, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(torch.from_numpy(X).to(gpu), Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))


@pytest.mark.parametrize("alg", [0, 1, 2])
def test_vendor_rocsparse_comparator(gpu, alg):
    """The rocSPARSE comparator (PETSc-block analogue) agrees with the
    reference's sequential result under the reference's own check
    (areMatricesEqual, 1e-6 absolute, SC/utils.cpp:55) and 1e-12 relative."""
    A = smfv.gen_fem27(3000, 12, 12, 0.8, 3)
    K = 32
    X = smfv.generateLargeFatVector(A.numCols, K)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    v = smfv.VendorSpmm(dA, dX, Y, alg=alg)
    v.run()
    torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    assert np.all(np.abs(Yh - Yref) <= 1e-12 * scale + 1e-300)
    assert np.max(np.abs(Yh - Yref)) <= 1e-6


def test_tiled_plan_fma_within_tolerance(gpu):
    """Opt-in SMFV_PLAN_FMA: same per-row order, fused multiply-add; within
    1e-12 x sum|a||x| of the reference (the north star allows 1e-6 relative)."""
    A = smfv.gen_fem27(5000, 12, 12, 0.83, 7)
    K = 64
    X = np.random.default_rng(7).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    dA = smfv.DeviceCSR(A, gpu)
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", fma=True)
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(torch.from_numpy(X).to(gpu), Y)
    torch.cuda.synchronize()
    assert np.all(np.abs(Y.cpu().numpy() - Yref) <= 1e-12 * scale + 1e-300)


def test_spmv_stream_k1(gpu):
    """K = 1 (k_spmv_stream): rows spanning many 2048-entry chunks, empty
    rows, a row block that starts mid-matrix and an unaligned leading
    dimension; bit-identical to the reference order."""
    m, n = 700, 50000
    lens = np.random.default_rng(11).integers(0, 40, m)
    lens[[3, 300]] = [9000, 20000]
    lens[[0, 1, 699]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(12)
    ci = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
    A = mat(rp, ci, rng.uniform(-1, 1, rp[-1]), m, n)
    X = rng.uniform(-1, 1, (n, 1))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    for v in (smfv.Variant.SEQUENTIAL, smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE):
        assert np.array_equal(bits(run(v, A, X, gpu)), bits(Yref)), v
        assert np.array_equal(bits(run(v, A, X, gpu, 1, 3)), bits(Yref)), v
    dA = smfv.DeviceCSR(A, gpu)
    Y = torch.full((m, 1), np.nan, dtype=torch.float64, device=gpu)
    S.spmm_rowblock(dA, 250, 650, torch.from_numpy(X).to(gpu), Y[250:650])
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y[250:650].cpu().numpy()), bits(Yref[250:650]))


def _chunk_matrix(seed, m=9000, n=200000):
    """Rows for the K = 1 chunk plan's edges: empty rows, runs of 300 short
    rows (more rows than a chunk's 256 lanes), rows of exactly 1,024 and
    1,023 entries (a whole chunk), a sliding column band (every row spans
    < 2^16) that jumps back for rows 6000-6009 (chunks end on the span)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 48, m)
    lens[100:400] = rng.integers(0, 3, 300)
    lens[[0, 1, 2, m - 1]] = 0
    lens[[500, 501, 4000]] = [1024, 1023, 1024]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = []
    for r, L in enumerate(lens):
        lo = 0 if 6000 <= r < 6010 else r * (n - 60000) // m
        ci.append(np.sort(rng.choice(np.arange(lo, lo + 60000), L, replace=False)))
    return mat(rp, np.concatenate(ci).astype(np.int32), rng.uniform(-1, 1, rp[-1]), m, n)


@pytest.mark.parametrize("K", [2, 3, 4, 5, 8, 12, 16, 31])
def test_narrow_k_column_window(gpu, K):
    """1 < K < 32 (a ColumnWise rank's K/p window, SC/...ColumnWise.cpp:34-48):
    the untiled row kernel, bit-identical to the reference's sequential sum
    for every variant but NONZERO (merge path, 1e-12) on the chunk test
    pattern (empty rows, a row spanning > 2^16 columns), read from a column
    window of a wider X (X + f, the full row stride) into a padded Y."""
    A = _chunk_matrix(71 + K)
    Kx = 40
    X = np.random.default_rng(72 + K).uniform(-1, 1, (A.numCols, Kx))
    dA = smfv.DeviceCSR(A, gpu)
    dXf = torch.from_numpy(X).to(gpu)
    absA = np.abs(A.values)
    for f in (0, 7):  # column window [f, f + K) of the 40-wide X
        Xw = np.ascontiguousarray(X[:, f:f + K])
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, Xw)
        for v in smfv.Variant:
            plan = smfv.SpmmPlan(v, dA, K)
            Yb = torch.full((A.numRows, K + 3), np.nan, dtype=torch.float64, device=gpu)
            plan.run(dXf[:, f:f + K], Yb[:, :K])
            torch.cuda.synchronize()
            Y = Yb[:, :K].cpu().numpy()
            if v == smfv.Variant.NONZERO:
                scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, absA, np.abs(Xw))
                assert rel_err(Y, Yref, scale) <= NNZ_TOL, (v, f)
            else:
                assert np.array_equal(bits(Y), bits(Yref)), (v, f)
            assert torch.isnan(Yb[:, K:]).all()


def test_spmv_chunk_plan_k1(gpu):
    """K = 1 plans take the chunk layout (k_spmv_chunks: 16-bit column
    offsets, values snapshot, no row_ptr round trip) wherever the pattern
    fits it -- bit-identical to the reference's sequential sum for every
    variant, unaligned leading dimensions, row blocks and after an in-place
    value change; a row spanning more than 2^16 columns switches the plan to
    32-bit columns, a row longer than a chunk keeps it on k_spmv_stream."""
    A = _chunk_matrix(61)
    X = np.random.default_rng(62).uniform(-1, 1, (A.numCols, 1))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for v in (smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE, smfv.Variant.NONZERO):
        plan = smfv.SpmmPlan(v, dA, 1)
        st = plan.stats()
        assert st["tiled"] and st["tiles"] >= A.nnz // 2048, (v, st)
        for pads in ((0, 0), (1, 3)):
            Xb = torch.zeros((A.numCols, 1 + pads[0]), dtype=torch.float64, device=gpu)
            Xb[:, :1] = dX
            Yb = torch.full((A.numRows, 1 + pads[1]), np.nan, dtype=torch.float64, device=gpu)
            plan.run(Xb[:, :1], Yb[:, :1])
            torch.cuda.synchronize()
            assert np.array_equal(bits(Yb[:, :1].cpu().numpy()), bits(Yref)), (v, pads)
            if pads[1]:
                assert torch.isnan(Yb[:, 1:]).all()
    for r0, r1 in ((0, 9000), (450, 4100), (8990, 9000), (77, 77)):
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, 1, rows=(r0, r1))
        Y = torch.full((r1 - r0, 1), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dX, Y)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref[r0:r1])), (r0, r1, plan.stats())
        assert plan.stats()["tiled"] == (r1 > r0)
    # the matrix's cached plan re-binds after an in-place value change
    Y = torch.empty((A.numRows, 1), dtype=torch.float64, device=gpu)
    S.spmm(smfv.Variant.ROWWISE, dA, dX, Y)
    dA.values.mul_(-3.0)
    S.spmm(smfv.Variant.ROWWISE, dA, dX, Y)
    torch.cuda.synchronize()
    Y3 = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values * -3.0, X)
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Y3))
    # a row spanning > 2^16 columns: the wide layout; a row over a chunk: untiled
    rp = np.array([0, 3, 1003, 1006], np.int32)
    wide = mat(rp, np.concatenate([[0, 1, 2], np.arange(1000) * 79, [5, 70000, 70001]]).astype(np.int32),
               np.random.default_rng(63).uniform(-1, 1, 1006), 3, 80000)
    long_row = mat(np.array([0, 1100], np.int32), np.arange(1100, dtype=np.int32),
                   np.random.default_rng(64).uniform(-1, 1, 1100), 1, 2000)
    for B, tiled in ((wide, True), (long_row, False)):
        XB = np.random.default_rng(65).uniform(-1, 1, (B.numCols, 1))
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(B, gpu), 1)
        assert plan.stats()["tiled"] == tiled
        Y = torch.empty((B.numRows, 1), dtype=torch.float64, device=gpu)
        plan.run(torch.from_numpy(XB).to(gpu), Y)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y.cpu().numpy()), bits(oracle.spmm("sequential", B.rowPtr, B.colIndices,
                                                                       B.values, XB)))


def _forced_plan_matrix(seed):
    """fem27 rows plus a few rows too wide for a tile (direct rows)."""
    A = smfv.gen_random_rows(6000, 5000, 16, 2.0, 1500, seed)
    assert np.diff(A.rowPtr).max() > 448  # some rows go to the direct list
    return A


@pytest.mark.parametrize("rows", [(0, 6000), (1234, 4321), (5990, 6000), (100, 100)])
def test_plan_rowblock_tiled(gpu, rows):
    """smfv_plan_create_rows: a rank's row block (SC/...RowWise.cpp:36-50) as
    a tiled plan (direct rows included) -- bit-identical to the reference's
    rows [begin, end)."""
    A = _forced_plan_matrix(41)
    K = 64
    X = np.random.default_rng(41).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    r0, r1 = rows
    for tiles in ("force", "off"):
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles=tiles, rows=rows)
        Y = torch.full((r1 - r0, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(torch.from_numpy(X).to(gpu), Y)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref[r0:r1])), (tiles, plan.stats())
        if tiles == "force" and r1 > r0:
            assert plan.stats()["tiled"] and plan.stats()["row_begin"] == r0


def test_plan_bind_on_other_stream(gpu):
    """a tiled plan bound on one stream and run on a fresh stream
    with no synchronisation in between waits for the values snapshot."""
    A = _forced_plan_matrix(43)
    K = 32
    X = torch.from_numpy(np.random.default_rng(43).uniform(-1, 1, (A.numCols, K))).to(gpu)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X.cpu().numpy())
    dA = smfv.DeviceCSR(A, gpu)
    torch.cuda.synchronize()
    s_bind, s_run = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s_bind):
            torch.cuda._sleep(2_000_000)  # keep the bind stream busy: the gather runs late
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", stream=s_bind)
        Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(X, Y, stream=s_run)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))


def test_plan_values_snapshot_contract(gpu):
    """ADVICE r1 / include/smfv.h values contract: an explicit tiled plan
    computes with the values bound last -- for the tiles AND the direct rows
    (no mixing) -- until values_changed() re-binds; then it sees the new
    values.  The matrix's cached plans (spmm) re-bind on their own."""
    A = _forced_plan_matrix(47)
    K = 32
    X = np.random.default_rng(47).uniform(-1, 1, (A.numCols, K))
    Y_old = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    A2 = smfv.SparseMatrix(A.values * 2.0 - 0.25, A.colIndices, A.rowPtr, A.numRows, A.numCols)
    Y_new = oracle.spmm("sequential", A2.rowPtr, A2.colIndices, A2.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    dA.plan(smfv.Variant.ROWWISE, K)  # the cached (auto) plan
    forced = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force")
    assert forced.stats()["tiled"] and forced.stats()["direct_rows"] > 0
    dA._plans[("forced", K)] = forced
    dA.values.mul_(2.0).sub_(0.25)  # in place, same address, no re-bind
    Y = torch.empty((A.numRows, K), dtype=torch.float64, device=gpu)
    forced.run(dX, Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Y_old))  # the bound snapshot, all rows
    # the matrix's cached plan (spmm) re-binds by itself after an
    # in-place change torch has seen (the tensor's version counter moved)
    assert np.array_equal(bits(smfv.spmm(smfv.Variant.ROWWISE, dA, dX).cpu().numpy()), bits(Y_new))
    dA.values_changed()
    forced.run(dX, Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Y_new))
    # the cached plan (through spmm) sees the new values too
    assert np.array_equal(bits(smfv.spmm(smfv.Variant.ROWWISE, dA, dX).cpu().numpy()), bits(Y_new))


def test_dist_plan_single_rank(gpu):
    """Distributed plans (smfv_dist_plan_*) at one rank: every variant and
    mode, the rank-local share tiled where it pays; plus the row-partitioned
    plan (config 5's layout).  The exchange schedule is empty at p = 1; its
    p > 1 form is replayed over gloo in test_dist_gloo.py."""
    from sparsematrixmultiplicationmpi_amd import dist as D
    comm = D.Communicator(0, 1, D.Communicator.new_unique_id())
    A = smfv.gen_fem27(5000, 12, 12, 0.83, 53)
    K = 32
    X = np.random.default_rng(53).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for v in (smfv.Variant.ROWWISE, smfv.Variant.COLUMNWISE, smfv.Variant.NONZERO):
        for to_all in (False, True):
            for tiles in ("auto", "force"):
                P = D.DistPlan(comm, v, dA, K, to_all, tiles=tiles)
                Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
                P.run(dX, Y)
                torch.cuda.synchronize()
                Yh = Y.cpu().numpy()
                if v == smfv.Variant.NONZERO:
                    assert np.max(np.abs(Yh - Yref)) <= 1e-10
                else:
                    assert np.array_equal(bits(Yh), bits(Yref)), (v, to_all, tiles)
                    if tiles == "force":
                        assert P.stats()["tiled"]
    P = D.DistPlan(comm, smfv.Variant.ROWWISE, dA, K, True, tiles="force", rowpart=True, m=A.numRows)
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    P.run_local(dX, Y)
    P.exchange(Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))
    comm.close()


def test_dist_plan_chunked_single_rank(gpu):
    """(r5) A chunked ROWWISE distributed plan (SMFV_DIST_CHUNKS: one tiled
    row-block plan per chunk; each chunk's exchange waits for it on the
    plan's exchange stream, the caller's stream joins the last) on a
    one-rank communicator: bit-identical eager and inside a captured
    hipGraph (the fork to the exchange stream and the join back are
    captured), under both row partitions, with a values change re-bound."""
    from sparsematrixmultiplicationmpi_amd import dist as D
    comm = D.Communicator(0, 1, D.Communicator.new_unique_id())
    A = smfv.gen_fem27(9000, 14, 14, 0.83, 61)
    K = 32
    X = np.random.default_rng(61).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.from_numpy(X).to(gpu)
    for partition in ("balanced", "reference"):
        for chunks in (2, 3, 7):
            for to_all in (False, True):
                P = D.DistPlan(comm, smfv.Variant.ROWWISE, dA, K, to_all, tiles="force", partition=partition,
                               chunks=chunks)
                assert P.shape() == (1, 0, chunks) and P.stats()["tiled"]
                Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
                P.run(dX, Y)
                torch.cuda.synchronize()
                assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref)), (partition, chunks, to_all)
                Y.fill_(np.nan)
                g = torch.cuda.CUDAGraph()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    with torch.cuda.graph(g, stream=side):
                        P.run(dX, Y, stream=side)
                torch.cuda.current_stream().wait_stream(side)
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref)), ("graph", partition, chunks, to_all)
                del g
    # values changed in place: the chunk plans re-bind together
    dA.values.mul_(2.0)
    A2 = smfv.SparseMatrix(A.values * 2.0, A.colIndices, A.rowPtr, A.numRows, A.numCols)
    Y2ref = oracle.spmm("sequential", A2.rowPtr, A2.colIndices, A2.values, X)
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    P.run(dX, Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Y2ref))
    del P
    comm.close()


def test_columnwise_single_pass_k128(gpu):
    """COLUMNWISE on one device: every K panel of a row in one pass over its
    CSR (no per-panel re-launch); bit-identical at K = 8, 40 (odd panel
    split) and 128, with and without the tiled plan."""
    A = smfv.gen_fem27(4000, 12, 12, 0.83, 59)
    for K in (8, 40, 128):
        X = np.random.default_rng(K).uniform(-1, 1, (A.numCols, K))
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
        assert np.array_equal(bits(run(smfv.Variant.COLUMNWISE, A, X, gpu)), bits(Yref)), K


def test_permuted_cop20k_surrogate(gpu):
    """The cop20k_A surrogate under a random symmetric permutation (the same
    matrix, another numbering): the plan still tiles it (re-use estimated in
    the full pattern) and the result is bit-identical to the reference."""
    A = smfv.cop20k_surrogate()
    perm = np.random.default_rng(2024).permutation(A.numRows)
    B = smfv.inputs.permute_symmetric(A, perm)
    K = 32
    X = smfv.generateLargeFatVector(B.numCols, K)
    Yref = oracle.spmm("sequential", B.rowPtr, B.colIndices, B.values, X)
    dB = smfv.DeviceCSR(B, gpu)
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dB, K)
    st = plan.stats()
    assert st["tiled"] and st["est_reuse"] >= 3.0 and st["reuse"] >= 5.0, st
    Y = torch.full((B.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(torch.from_numpy(X).to(gpu), Y)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref))


@pytest.mark.parametrize("K", [32, 128])
def test_mfma_tile_kernel_within_tolerance(gpu, K):
    """Opt-in SMFV_PLAN_MFMA (k_rows_mfma, config 3's MFMA K-panel):
    dense 16 x 4 blocks on v_mfma_f64_16x16x4f64, reassociated sums, within
    1e-12 x sum|a||x| of the reference; a row with a repeated column (the
    pat4x6 duplicate) goes to the direct list and stays exact."""
    for A in (smfv.gen_fem27(5000, 12, 12, 0.83, 61),
              smfv.readMatrixMarketFile(__import__("os").path.join(__import__("os").path.dirname(__file__),
                                                                   "golden", "pat4x6.mtx"))):
        X = np.random.default_rng(K).uniform(-1, 1, (A.numCols, K))
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
        scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(A, gpu), K, tiles="force", mfma=True)
        assert plan.stats()["mfma"]
        Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(torch.from_numpy(X).to(gpu), Y)
        torch.cuda.synchronize()
        assert np.all(np.abs(Y.cpu().numpy() - Yref) <= 1e-12 * scale + 1e-300)


def test_mfma_tile_kernel_full_size_k128(gpu):
    """(r5) The MFMA opt-in on BASELINE config 3 at full size (cop20k_A
    surrogate, K = 128; VERDICT r4 weak 1: it was checked only at 5k rows):
    within 1e-12 x sum|a||x| of the reference order, every row written."""
    A = smfv.cop20k_surrogate()
    K = 128
    X = smfv.generateLargeFatVector(A.numCols, K)
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    scale = oracle.spmm("sequential", A.rowPtr, A.colIndices, np.abs(A.values), np.abs(X))
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(A, gpu), K, tiles="force", mfma=True)
    assert plan.stats()["mfma"]
    Y = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(torch.from_numpy(X).to(gpu), Y)
    torch.cuda.synchronize()
    Yh = Y.cpu().numpy()
    assert np.isfinite(Yh).all()
    assert np.all(np.abs(Yh - Yref) <= 1e-12 * scale + 1e-300)


# ---------------------------------------------------------------------------
# (r5) live values (SMFV_PLAN_LIVE_VALUES): the tiled kernel's loaders DMA the
# value pairs straight from the caller's CSR values -- no snapshot, no bind.
# Bit-identical to the reference; a row of odd length reads one value past
# its end (the next row's first, or past the block through a range-checked
# buffer: 0), which its team overwrites with -0.0 before summing, so even a
# NaN / inf in the next row stays out of it.
# ---------------------------------------------------------------------------
def _live_run(A, X, gpu, K=None, rows=None, live=True, tiles="force", Xd=None):
    dA = smfv.DeviceCSR(A, gpu)
    K = X.shape[1] if K is None else K
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(gpu) if Xd is None else Xd
    m = A.numRows if rows is None else rows[1] - rows[0]
    plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles=tiles, rows=rows, live_values=live)
    Y = torch.full((m, K), np.nan, dtype=torch.float64, device=gpu)
    plan.run(Xd, Y)
    torch.cuda.synchronize()
    return plan, Y.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_live_values_golden(gpu, name):
    g = load_golden(name)
    A = mat(g["row_ptr"], g["col_idx"], g["values"], g["m"], g["n"])
    K = g["X"].shape[1]
    plan, Y = _live_run(A, g["X"], gpu)
    if K % 32 == 0 or K in (4, 8, 16):
        assert plan.stats()["live_values"] and plan.stats()["snapshot_entries"] == 0
    assert np.array_equal(bits(Y), bits(g["Y_seq"])), name


@pytest.mark.parametrize("K", [4, 8, 16, 32, 64, 128])
def test_live_values_odd_rows_and_block_end(gpu, K):
    """Odd row lengths everywhere (1..41), the last row odd with nnz odd (its
    pair's second half lies past the array: the buffer's range check gives
    0), NaN and inf as the first value of rows that follow odd rows (never in
    the odd row's sum), and row blocks starting at odd CSR indices."""
    rng = np.random.default_rng(100 + K)
    m = n = 2600
    lens = (np.arange(m) * 7) % 41 + 1
    lens[-1] = 13
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    if rp[-1] % 2 == 0:
        lens[-2] += 1
        rp[1:] = np.cumsum(lens)
    assert rp[-1] % 2 == 1
    ci = np.concatenate([np.sort(rng.choice(np.arange(max(0, i - 50), min(n, i + 50)), L, replace=False))
                         for i, L in enumerate(lens)]).astype(np.int32)
    va = rng.uniform(-1, 1, ci.size)
    bad = [i for i in range(1, m) if lens[i - 1] % 2 == 1][:40:3]
    va[rp[bad[::2]]] = np.nan
    va[rp[bad[1::2]]] = np.inf
    A = mat(rp.astype(np.int32), ci, va, m, n)
    X = rng.uniform(-1, 1, (n, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)

    def same(Y, Yr):  # bit for bit where finite; NaN exactly where the reference has NaN
        nan = np.isnan(Yr)
        return np.array_equal(np.isnan(Y), nan) and np.array_equal(bits(Y)[~nan], bits(Yr)[~nan])
    plan, Y = _live_run(A, X, gpu)
    assert plan.stats()["live_values"] and plan.stats()["tiled"]
    assert same(Y, Yref)
    odd = [r for r in range(1, m) if rp[r] % 2 == 1]
    for r0, r1 in ((odd[0], 1500), (odd[len(odd) // 2], m), (odd[-1] - 200, m - 1)):
        plan, Yb = _live_run(A, X, gpu, rows=(r0, r1))
        assert same(Yb, Yref[r0:r1]), (r0, r1)


@pytest.mark.parametrize("K", [32, 8])
def test_live_values_poison_before_odd_rows(gpu, K):
    """(r6) NaN and -inf as the LAST value of rows followed by rows that start
    at odd CSR indices (whose value pairs are 8-byte aligned; an r6 variant
    that started them one value early, 16-byte aligned, read exactly these
    values into its first pair -- measured even and dropped,
    profiles/r06/lead/): the poisoned rows are NaN, their neighbours bit-exact.
    Row lengths 1..41, row blocks starting at odd and even CSR indices."""
    rng = np.random.default_rng(200 + K)
    m = n = 2600
    lens = (np.arange(m) * 5) % 41 + 1
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(np.arange(max(0, i - 50), min(n, i + 50)), L, replace=False))
                         for i, L in enumerate(lens)]).astype(np.int32)
    va = rng.uniform(-1, 1, ci.size)
    lead_rows = [r for r in range(1, m) if rp[r] % 2 == 1 and lens[r] % 8]
    assert len(lead_rows) > 500
    poison = lead_rows[:60:2]
    va[rp[poison[::2]] - 1] = np.nan   # the last value of the row before
    va[rp[poison[1::2]] - 1] = -np.inf
    A = mat(rp.astype(np.int32), ci, va, m, n)
    X = rng.uniform(-1, 1, (n, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)

    def same(Y, Yr):
        nan = np.isnan(Yr)
        return np.array_equal(np.isnan(Y), nan) and np.array_equal(bits(Y)[~nan], bits(Yr)[~nan])
    assert np.all(np.isfinite(Yref[poison]))  # the poisoned values belong to the rows before
    plan, Y = _live_run(A, X, gpu)
    assert plan.stats()["live_values"] and plan.stats()["tiled"]
    assert same(Y, Yref)
    for r0, r1 in ((poison[3], 1900), (poison[4] + 1, m), (1, m - 3)):
        plan, Yb = _live_run(A, X, gpu, rows=(r0, r1))
        assert same(Yb, Yref[r0:r1]), (r0, r1, int(rp[r0]) % 2)


def test_live_values_full_size_and_contract(gpu):
    """The cop20k_A stand-ins at K = 32 and the stencil at K = 128: live
    plans bit-identical; values changed IN PLACE with no bind are seen by the
    next execute (live semantics: a bind is a no-op); inside a captured graph
    too; and the live plan holds no snapshot."""
    for A, K in ((smfv.cop20k_surrogate(), 32), (smfv.inputs.cop20k_irregular_surrogate(), 32),
                 (smfv.cop20k_surrogate(), 128)):
        X = smfv.generateLargeFatVector(A.numCols, K)
        dA = smfv.DeviceCSR(A, gpu)
        dX = torch.from_numpy(X).to(gpu)
        live = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, live_values=True)
        snap = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K)
        st, ss = live.stats(), snap.stats()
        assert st["live_values"] and st["tiled"] and st["tiles"] == ss["tiles"] and st["snapshot_entries"] == 0
        Yl = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        Ys = torch.full_like(Yl, np.nan)
        live.run(dX, Yl)
        snap.run(dX, Ys)
        torch.cuda.synchronize()
        assert torch.equal(Yl.view(torch.int64), Ys.view(torch.int64))
        if K == 32 and A.numRows == 121192:
            Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
            assert np.array_equal(bits(Yl.cpu().numpy()), bits(Yref))
        # in place, no bind: the live plan's next execute reads the new values
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                rp, ci, va = dA.ptrs()
                smfv._lib.call("smfv_plan_execute", live._plan, rp, ci, va, dX.data_ptr(), K, Yl.data_ptr(), K,
                               S.stream_handle(side))
        torch.cuda.current_stream().wait_stream(side)
        dA.values.mul_(-0.5)
        torch.cuda.synchronize()
        g.replay()
        snap.bind_values()  # (the snapshot plan needs its bind)
        snap.run(dX, Ys)
        torch.cuda.synchronize()
        assert torch.equal(Yl.view(torch.int64), Ys.view(torch.int64))
        del g


def test_live_values_x_over_4gib(gpu):
    """(r6) A live-values tiled plan executed on an X spanning
    4 GiB or more (n * ldx * 8; known only at execute) runs the untiled row
    kernel on the same live values instead of failing: bit-identical to the
    untiled plan, and to the snapshot plan (whose non-SADDR instance takes
    such an X).  A 27-point stencil of 4,000 rows whose X has 16.8 M rows
    (4.3 GB).  Its columns are spread over all of X: c -> c * (n // 4000) for
    c < 3,000 (byte offsets up to 3.2 GB) and the last 1,000 onto the last
    1,000 rows of X, all of which start beyond 4 GiB (c * (n // 4000) alone
    ends 1.4 MB short of 2^32).  All three plans are compared with a host loop
    (adversarial.ref_f64) over the 4,000 X rows referenced, copied back from
    the device -- fill_x_hash's values are small integers -- and with one
    another."""
    import adversarial as adv
    B = smfv.gen_fem27(4000, 16, 16, 0.83, 7)
    K = 32
    n = (1 << 32) // (8 * K) + 1024
    c = np.arange(4000, dtype=np.int64)
    cmap = np.where(c < 3000, c * (n // 4000), n - 4000 + c)
    assert np.all(np.diff(cmap) > 0) and cmap[-1] == n - 1
    assert 1 << 31 < cmap[2999] * K * 8 < 1 << 32 <= cmap[3000] * K * 8
    cols = cmap[B.colIndices].astype(np.int32)
    assert np.mean(cols.astype(np.int64) * K * 8 >= 1 << 32) > 0.2
    A = smfv.SparseMatrix(B.values, cols, B.rowPtr, B.numRows, n)
    dA = smfv.DeviceCSR(A, gpu)
    dX = torch.empty((n, K), dtype=torch.float64, device=gpu)
    smfv.fill_x_hash(dX, 11)
    Xh = dX[torch.from_numpy(cmap).to(gpu)].cpu().numpy()
    assert np.all(Xh == np.rint(Xh)) and Xh.min() >= 1 and Xh.max() <= 100 and len(np.unique(Xh)) > 50
    small = adv.Csr(np.asarray(B.values), np.asarray(B.colIndices), np.asarray(B.rowPtr), B.numRows, 4000)
    Yref = adv.ref_f64(small, Xh)
    live = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, live_values=True, tiles="force")
    snap = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force")
    ref = smfv.SpmmPlan(smfv.Variant.SEQUENTIAL, dA, K, tiles="off")
    assert live.stats()["live_values"] and live.stats()["tiled"]
    assert snap.stats()["tiled"] and not snap.stats()["live_values"] and not ref.stats()["tiled"]
    Y = {k: torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu) for k in ("live", "snap", "ref")}
    live.run(dX, Y["live"])
    snap.run(dX, Y["snap"])
    ref.run(dX, Y["ref"])
    torch.cuda.synchronize()
    for k in Y:
        assert np.array_equal(bits(Y[k].cpu().numpy()), bits(Yref)), k
    assert torch.equal(Y["live"].view(torch.int64), Y["ref"].view(torch.int64))
    assert torch.equal(Y["snap"].view(torch.int64), Y["ref"].view(torch.int64))
    # the live values are read at every execute (no bind)
    dA.values.mul_(-0.25)
    live.run(dX, Y["live"])
    ref.run(dX, Y["ref"])
    torch.cuda.synchronize()
    assert torch.equal(Y["live"].view(torch.int64), Y["ref"].view(torch.int64))
    small.values = -0.25 * small.values
    assert np.array_equal(bits(Y["live"].cpu().numpy()), bits(adv.ref_f64(small, Xh)))
    del dX


@pytest.mark.parametrize("K", [4, 8])
def test_narrow_team_tiles(gpu, K):
    """(r5) K = 4 / 8 windows take the narrow-team tiles (k_rows_wsn: K/2
    lanes per row, 256 / 128-row tiles, window-only X image with u16
    offsets): bit-identical to the reference's order, into a padded Y (the
    padding stays NaN), with direct rows; and identical to the k_rows_ws
    NARROW form (tiled_kernel="ws", the A/B); on both cop20k stand-ins at
    full size and on short / empty rows beside long ones."""
    from conftest import short_rows_band
    rng = np.random.default_rng(200 + K)
    mats = [smfv.gen_fem27(9000, 14, 14, 0.83, K), smfv.gen_random_rows(7000, 6000, 16, 2.0, 1500, K),
            smfv.cop20k_surrogate(), smfv.inputs.cop20k_irregular_surrogate(),
            # (r5) trimmed batches: rows of 0-7 entries beside 30-60 (empty rows,
            # every length residue), and a tile with empty team slots
            short_rows_band(6000, 31 + K), short_rows_band(77, 5 + K, long_every=9)]
    for A in mats:
        X = rng.uniform(-1, 1, (A.numCols, 32))
        dA = smfv.DeviceCSR(A, gpu)
        dXf = torch.from_numpy(X).to(gpu)
        f = 32 - K - 4
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, np.ascontiguousarray(X[:, f:f + K]))
        for tk in ("auto", "ws"):
            plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", tiled_kernel=tk)
            st = plan.stats()
            assert st["tiled"] and st["kernel"] == ("k_rows_wsn" if tk == "auto" else "k_rows_ws"), st
            Yb = torch.full((A.numRows, K + 3), np.nan, dtype=torch.float64, device=gpu)
            plan.run(dXf[:, f:f + K], Yb[:, :K])
            torch.cuda.synchronize()
            assert np.array_equal(bits(Yb[:, :K].cpu().numpy()), bits(Yref)), (A.numRows, tk, st)
            assert torch.isnan(Yb[:, K:]).all()
        # values changed: the snapshot re-binds (per-entry gather) and the sums follow
        dA.values.mul_(0.25)
        plan = smfv.SpmmPlan(smfv.Variant.COLUMNWISE, dA, K, tiles="force")
        Yb = torch.full((A.numRows, K), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dXf[:, f:f + K], Yb)
        torch.cuda.synchronize()
        Y4 = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values * 0.25, np.ascontiguousarray(X[:, f:f + K]))
        assert np.array_equal(bits(Yb.cpu().numpy()), bits(Y4))


@pytest.mark.parametrize("tk", ["auto", "ws2", "ws3"])
def test_row_pair_tiles(gpu, tk):
    """(r5) Row pairs: teams summing a second (short) row after their first
    (SMFV_PLAN_ROW_PAIRS; SMFV_PLAN_SINGLE_ROWS keeps one row per team;
    neither: the plan with fewer rounds of tiles per block) -- on a
    0-7-entry band with long rows (every residue, empty rows), a row block
    starting mid-matrix and the irregular cop20k_A stand-in; K = 32 / 64 /
    128 and a 16-column window of a wider X (NARROW): bit-identical to the
    reference's order and to the single-row plan, and after a value change
    (the bind items re-gather the paired rows' values); live-values plans
    pair rows too (odd-length second rows: their -0.0 write)."""
    from conftest import short_rows_band
    rng = np.random.default_rng(300)
    mats = [short_rows_band(20000, 3)] + ([smfv.inputs.cop20k_irregular_surrogate()] if tk == "auto" else [])
    for A in mats:
        dA = smfv.DeviceCSR(A, gpu)
        X = rng.uniform(-1, 1, (A.numCols, 128))
        dXf = torch.from_numpy(X).to(gpu)
        for K, f, rows in ((32, 0, None), (64, 32, None), (128, 0, None), (16, 8, None), (32, 0, (777, 15000))):
            Xw = np.ascontiguousarray(X[:, f:f + K])
            r0, r1 = rows or (0, A.numRows)
            Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, Xw)[r0:r1]
            outs = []
            for pairs, live in (("on", False), ("off", False), ("on", True), ("auto", False)):
                plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, K, tiles="force", rows=rows, row_pairs=pairs,
                                     tiled_kernel="auto" if tk == "auto" else tk, live_values=live)
                st = plan.stats()
                assert st["tiled"] and st["kernel"] == "k_rows_ws" and st["live_values"] == live, st
                if pairs != "auto":
                    assert (st["paired_rows"] > 0) == (pairs == "on"), st
                Yb = torch.full((r1 - r0, K + 1), np.nan, dtype=torch.float64, device=gpu)
                plan.run(dXf[:, f:f + K], Yb[:, :K])
                torch.cuda.synchronize()
                outs.append(Yb[:, :K].cpu().numpy())
                assert np.array_equal(bits(outs[-1]), bits(Yref)), (K, f, rows, single, st)
                assert torch.isnan(Yb[:, K:]).all()
        # values changed: a re-bind gathers the paired rows' values too
        dA.values.mul_(-0.5)
        plan = smfv.SpmmPlan(smfv.Variant.ROWWISE, dA, 32, tiles="force", row_pairs="on")
        dA.values.mul_(-2.0)
        plan.bind_values()
        Y = torch.full((A.numRows, 32), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dXf[:, :32], Y)
        torch.cuda.synchronize()
        Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, np.ascontiguousarray(X[:, :32]))
        assert np.array_equal(bits(Y.cpu().numpy()), bits(Yref)), plan.stats()
    if tk == "auto":  # the automatic choice: the irregular stand-in pairs (10 -> 8 rounds), the stencil does not
        irr = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(mats[1], gpu), 32).stats()
        sten = smfv.SpmmPlan(smfv.Variant.ROWWISE, smfv.DeviceCSR(smfv.cop20k_surrogate(), gpu), 32).stats()
        assert irr["paired_rows"] > 0 and sten["paired_rows"] == 0, (irr, sten)


def test_row_pairs_every_variant(gpu):
    """(r5) Row pairs under every variant's single-device plan (SEQUENTIAL,
    ROWWISE, COLUMNWISE, NONZERO over whole rows: the same tiled kernel,
    bit-identical to the reference's order) and at K = 64 with a padded Y
    (an even row stride: an odd one sends every plan to the untiled kernels,
    and NONZERO's to the merge path, pick_vec)."""
    from conftest import short_rows_band
    A = short_rows_band(12000, 9)
    K = 64
    X = np.random.default_rng(9).uniform(-1, 1, (A.numCols, K))
    Yref = oracle.spmm("sequential", A.rowPtr, A.colIndices, A.values, X)
    dA, dX = smfv.DeviceCSR(A, gpu), torch.from_numpy(X).to(gpu)
    for v in smfv.Variant:
        plan = smfv.SpmmPlan(v, dA, K, tiles="force", row_pairs="on")
        st = plan.stats()
        assert st["tiled"] and st["paired_rows"] > 0, (v, st)
        Yb = torch.full((A.numRows, K + 6), np.nan, dtype=torch.float64, device=gpu)
        plan.run(dX, Yb[:, :K])
        torch.cuda.synchronize()
        assert np.array_equal(bits(Yb[:, :K].cpu().numpy()), bits(Yref)), (v, st)
        assert torch.isnan(Yb[:, K:]).all()
