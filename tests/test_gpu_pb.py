"""Propagation-blocking form (class 5, MgcgSetMatrixCompression mode 3) for matrices without locality: a lossless re-layout whose
row sums are formed in stored order, so every product, epilogue and solve must be bit-identical to the CSR kernels / the oracle."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.solver import ConjugateGradientParallelGpu, ConjugateGradientSingleGpu
from tests.gpu_util import DeviceCsr, Handles, dvec

pytestmark = pytest.mark.gpu

TILE = 16384
ROUND = 9088          # entries of a row block per round (kPbRoundCap)


def _info(sparse, idx=0):
    d, v, r, n = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong()
    cls = _lib.lib().MgcgAnalysisInfo(sparse, idx, C.byref(d), C.byref(v), C.byref(r), C.byref(n))
    return cls, d.value, v.value, r.value, n.value


@pytest.fixture
def reference_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    v = C.c_int(0)
    assert _lib.lib().MgcgGetTuning(b"dot_order", C.byref(v)) == 0 and v.value == 1
    return mgcg_env


@pytest.fixture(scope="module")
def small():
    return problems.random_spd(200_000, seed=12345)


def _largest_block(s):
    ro = np.asarray(s.RowOffsets, dtype=np.int64)
    starts = np.arange(0, s.Count, 1024)
    return int((ro[np.minimum(starts + 1024, s.Count)] - ro[starts]).max())


def _largest_piece(s):
    ro = np.asarray(s.RowOffsets, dtype=np.int64)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    tiles = (s.ColumnIndeces[: s.nnz] // TILE).astype(np.int64)
    return int(np.bincount((rows // 1024) * (tiles.max() + 1) + tiles).max())


def test_products_at_small_size(oracle, small):
    s = small
    assert _largest_block(s) > 65535            # 16-bit positions relative to the block would not do
    assert _largest_piece(s) > ROUND            # ... and a round may end inside a piece
    L = _lib.lib()
    h = Handles()
    A = DeviceCsr(s)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(s.Count)
    ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x)
    L.MgcgSetMatrixCompression(h.sparse, _lib.COMPRESSION_PB)
    got = A.spmv(h, x)
    cls, tiles, rounds, rows, nnz = _info(h.sparse)
    assert (cls, tiles, rows, nnz) == (5, 13, s.Count, s.nnz)
    assert rounds >= (_largest_block(s) + ROUND - 1) // ROUND
    assert np.array_equal(got, ref)
    assert np.array_equal(A.spmv(h, x, alpha=2.0), 2.0 * ref)
    y0 = rng.standard_normal(s.Count)
    assert np.array_equal(A.spmv(h, x, alpha=-1.5, beta=0.25, y0=y0), -1.5 * ref + 0.25 * y0)
    vx, vy = dvec(x), dvec(np.zeros(s.Count))
    dot = L.CsrMVDot(h.blas, h.sparse, vy.ToRawPtr(), A.e.ToRawPtr(), A.r.ToRawPtr(), A.c.ToRawPtr(), vx.ToRawPtr(), vx.ToRawPtr(), s.nnz, s.Count, s.Count)
    _lib.check("CsrMVDot")
    assert np.array_equal(vy.to_numpy(s.Count), ref)
    want = float(np.dot(x, ref))
    assert abs(dot - want) <= 1e-13 * abs(want)
    assert _info(h.sparse)[0] == 5
    h.close()


def _edge_matrix():
    """Empty rows, one row of several thousand entries over every tile, a column count that is not a multiple of the tile width and
    a last block shorter than 1024 rows; every other row a few entries spread uniformly (far from the diagonal)."""
    import scipy.sparse as sp

    n = 300_001                                  # (far enough apart that the sampled mean distance from the diagonal exceeds a tile)
    rng = np.random.default_rng(11)
    k = rng.integers(3, 9, size=n)
    k[np.arange(n) % 97 == 5] = 0
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=rows.shape[0])
    rows = np.concatenate([rows, np.full(6000, 150_000)])
    cols = np.concatenate([cols, rng.integers(0, n, size=6000)])
    key = np.unique(rows.astype(np.int64) * n + cols)
    rows, ci = key // n, (key % n).astype(np.int32)
    ro = np.zeros(n + 1, np.int64)
    ro[1:] = np.cumsum(np.bincount(rows, minlength=n))
    vals = rng.standard_normal(ci.shape[0])
    A = sp.csr_matrix((vals, ci, ro), shape=(n, n))
    return problems.LinearSystem(np.ascontiguousarray(A.data), np.ascontiguousarray(A.indices, dtype=np.int32),
                                 np.ascontiguousarray(A.indptr, dtype=np.int32), np.zeros(n), np.ones(n), "edge")


def _product(oracle, s, mode, seed=5):
    L = _lib.lib()
    h = Handles()
    A = DeviceCsr(s)
    x = np.random.default_rng(seed).standard_normal(s.Count)
    ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x)
    L.MgcgSetMatrixCompression(h.sparse, mode)
    got = A.spmv(h, x)
    cls = _info(h.sparse)[0]
    h.close()
    return cls, got, ref


def test_edge_cases_stay_exact(oracle):
    s = _edge_matrix()
    assert s.Count % 1024 != 0 and s.Count % TILE != 0 and (np.diff(s.RowOffsets) == 0).any()
    cls, got, ref = _product(oracle, s, _lib.COMPRESSION_PB)
    assert cls == 5 and np.array_equal(got, ref)


def test_unsorted_rows_are_declined_and_exact(oracle, mgcg_env, capfd):
    """Rows stored in reverse: the tiles of a row step back, so the stored-order sums cannot be kept -- declined, and the product is
    the CSR kernels' (not the column tiles' either: those need sorted rows too)."""
    mgcg_env.setenv("MGCG_VERBOSE", "1")
    s = problems.random_spd(199_999, seed=12345, sort_columns=False)
    assert (np.diff(s.ColumnIndeces[s.RowOffsets[5]: s.RowOffsets[6]]) < 0).all()
    cls, got, ref = _product(oracle, s, _lib.COMPRESSION_PB)
    assert "step back to an earlier column tile" in capfd.readouterr().err
    assert cls not in (4, 5)
    h = Handles()
    plain = DeviceCsr(s).spmv(h, np.random.default_rng(5).standard_normal(s.Count))     # compression off: the same CSR kernel
    h.close()
    assert np.array_equal(got, plain)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * np.abs(ref).max())


@pytest.mark.parametrize("builder", [lambda: problems.poisson(40, 40, 40), lambda: problems.mgcg_main(3000, 8)])
def test_matrices_with_locality_keep_the_mode_1_choice(oracle, builder):
    s = builder()
    c1, g1, ref = _product(oracle, s, _lib.COMPRESSION_BEST)
    c3, g3, _ = _product(oracle, s, _lib.COMPRESSION_PB)
    assert c1 == c3 and c3 != 5 and np.array_equal(g1, ref) and np.array_equal(g3, ref)


def test_solve_one_rank(oracle, small):
    s = small
    ref = oracle.cg(s, rule=oracle.RULE_CSHARP, max_iteration=2000)
    cg = ConjugateGradientSingleGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 2000, 1e-8, rule=_lib.RULE_CSHARP).load(s)
    _lib.lib().MgcgSetMatrixCompression(cg.cusparse, _lib.COMPRESSION_PB)
    cg.Initialize()
    cg.Solve()
    cg.Read()
    assert _info(cg.cusparse)[0] == 5
    assert cg.Iteration == ref["iteration"]
    assert np.abs(cg.x - ref["x"]).max() <= 1e-10 * np.abs(ref["x"]).max()
    cg.Dispose()


def test_solve_one_rank_in_the_reference_order(oracle, small, reference_order):
    s = small
    ref = oracle.cg(s, rule=oracle.RULE_CSHARP, max_iteration=2000, trace=True)
    cg = ConjugateGradientSingleGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 2000, 1e-8, rule=_lib.RULE_CSHARP).load(s)
    _lib.lib().MgcgSetMatrixCompression(cg.cusparse, _lib.COMPRESSION_PB)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    assert _info(cg.cusparse)[0] == 5
    assert cg.Iteration == ref["iteration"]
    assert np.array_equal(cg.trace, ref["trace"])
    assert np.array_equal(cg.x, ref["x"])
    cg.Dispose()


@pytest.mark.parametrize("devices", [1, 2])
def test_phase_driver_equals_the_multi_device_oracle(oracle, small, reference_order, devices):
    """The reference's phase driver multiplies through CsrMV / CsrMVDot / Solve0 / Solve1 (per-op products) on every device."""
    reference_order.setenv("MGCG_VIRTUAL_DEVICES", str(devices))
    reference_order.setenv("MGCG_COMPRESSION", "3")
    s = small
    ref = oracle.cg_parallel(s, devices, max_iteration=2000)
    cg = ConjugateGradientParallelGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 2000, 1e-8, deviceCount=devices).load(s)
    cg.Initialize()
    cg.Solve()
    cg.Read()
    assert _info(cg.cusparse[0])[0] == 5                     # (rank 0's rows reach far; a later slice may sample closer to its diagonal)
    assert cg.Iteration == ref["iteration"] and cg.Residual == ref["residual"]
    assert np.array_equal(cg.x, ref["x"])
    cg.Dispose()


def test_loopback_ranks(oracle, reference_order):
    from conjugategradient_amd.parallel import ConjugateGradientRankGpu
    from tests.test_gpu_parallel import _run_ranks_in_threads

    world = 3
    reference_order.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = problems.random_spd(150_000, seed=12345)
    ref = oracle.cg_parallel(s, world, max_iteration=2000)
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, 2000, 1e-8, rank=rank, world=world, comm=comm, device=rank).load(s)
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, _lib.COMPRESSION_PB)
        cg.Initialize()
        cg.Solve()
        cg.Read()
        out = (cg.part.offset, cg.part.count, cg.x[cg.part.offset: cg.part.offset + cg.part.count].copy(), cg.Iteration, _info(cg.cusparse)[0])
        cg.Dispose()
        return out

    x = np.zeros(s.Count)
    classes = []
    for off, cnt, xs, it, cls in _run_ranks_in_threads(world, make_rank):
        x[off: off + cnt] = xs
        classes.append((off, cls))
        assert it == ref["iteration"]
    # rank 0 takes the form over the global column range; the later slices of this matrix sample closer to their diagonal (the lower
    # triangle piles up near it: 8 K and 11 K columns at 150 K rows, under one tile) and keep the CSR kernels -- the ranks' forms differ
    # and the solve must not care
    assert dict(classes)[0] == 5, classes
    assert all(c in (0, 5) for _, c in classes), classes
    assert np.array_equal(x, ref["x"])


def test_writes_and_mode_switches_reanalyse(oracle, small):
    s = small
    L = _lib.lib()
    h = Handles()
    A = DeviceCsr(s)
    x = np.random.default_rng(8).standard_normal(s.Count)
    L.MgcgSetMatrixCompression(h.sparse, _lib.COMPRESSION_PB)
    assert np.array_equal(A.spmv(h, x), oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x))
    assert _info(h.sparse)[0] == 5
    L.Scal(h.blas, A.e.ToRawPtr(), 0.5, s.nnz)               # through the library: the form goes stale
    e2 = s.Elements[: s.nnz] * 0.5
    assert np.array_equal(A.spmv(h, x), oracle.spmv(e2, s.ColumnIndeces, s.RowOffsets, x))
    e3 = s.Elements[: s.nnz] * -3.0
    A.e.CopyFrom(e3, s.nnz)
    assert np.array_equal(A.spmv(h, x), oracle.spmv(e3, s.ColumnIndeces, s.RowOffsets, x))
    assert _info(h.sparse)[0] == 5
    # mode 1 has no form for this matrix (x spans fewer than 4 of class 4's tiles): the CSR kernels, the stored-order one here
    L.MgcgSetMatrixCompression(h.sparse, _lib.COMPRESSION_BEST)
    ref3 = oracle.spmv(e3, s.ColumnIndeces, s.RowOffsets, x)
    assert np.array_equal(A.spmv(h, x, kernel=1), ref3) and _info(h.sparse)[0] == 0
    L.MgcgSetMatrixCompression(h.sparse, _lib.COMPRESSION_PB)
    assert np.array_equal(A.spmv(h, x), ref3) and _info(h.sparse)[0] == 5
    L.MgcgSetMatrixCompression(h.sparse, _lib.COMPRESSION_BEST)
    assert np.array_equal(A.spmv(h, x, kernel=1), ref3) and _info(h.sparse)[0] == 0
    h.close()


def test_reinitialize_with_new_values_reanalyses(oracle, small):
    s = small
    cg = ConjugateGradientSingleGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 2000, 1e-8, rule=_lib.RULE_CSHARP).load(s)
    _lib.lib().MgcgSetMatrixCompression(cg.cusparse, _lib.COMPRESSION_PB)
    cg.Initialize()
    cg.Solve()
    cg.Read()
    it1 = cg.Iteration
    off = s.Elements[: s.nnz].copy()
    diag = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets)) == s.ColumnIndeces[: s.nnz]
    e2 = np.where(diag, off * 3.0, off)                      # a stronger diagonal: fewer iterations
    s2 = problems.LinearSystem(e2, s.ColumnIndeces.copy(), s.RowOffsets.copy(), np.zeros(s.Count), s.b.copy(), "random_spd x3 diagonal")
    ref2 = oracle.cg(s2, rule=oracle.RULE_CSHARP, max_iteration=2000)
    cg.A.Elements[: s.nnz] = e2
    cg.x[:] = 0.0
    cg.Initialize()
    cg.Solve()
    cg.Read()
    assert _info(cg.cusparse)[0] == 5
    assert ref2["iteration"] != it1 and cg.Iteration == ref2["iteration"]
    assert np.abs(cg.x - ref2["x"]).max() <= 1e-10 * np.abs(ref2["x"]).max()
    cg.Dispose()


def test_config5_at_full_size_class5(oracle):
    """BASELINE config 5 at 10 M rows under mode 3: the product equals the oracle's and the column-tile form's (mode 1) bit for bit,
    and the solve agrees with the class-4 solve."""
    from conjugategradient_amd.solver import VectorDouble, VectorInt

    s = problems.random_spd(10_000_000, mean_upper=14.0, seed=12345)
    N, nnz = s.Count, s.nnz
    L = _lib.lib()
    xs = np.cos(np.arange(N) * 0.01)
    ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, xs)
    cg = ConjugateGradientSingleGpu(N, int(np.diff(s.RowOffsets).max()), 0, 1000, 1e-8, rule=_lib.RULE_CSHARP)
    cg.A = type("M", (), {})()
    cg.A.Elements, cg.A.ColumnIndeces, cg.A.RowOffsets = s.Elements, s.ColumnIndeces, s.RowOffsets
    cg.vectorA.Dispose(); cg.vectorColumnIndeces.Dispose()
    cg.vectorA, cg.vectorColumnIndeces = VectorDouble(nnz), VectorInt(nnz)
    cg.x[:] = 0.0
    cg.b[:] = ref + 2.0
    cg.Initialize()
    dx, dy = VectorDouble(N), VectorDouble(N)
    dx.CopyFrom(xs, N)

    def product(mode):
        L.MgcgSetMatrixCompression(cg.cusparse, mode)
        L.CsrMV(cg.cusparse, cg.matDescr, dy.ToRawPtr(), cg.vectorA.ToRawPtr(), cg.vectorRowOffsets.ToRawPtr(), cg.vectorColumnIndeces.ToRawPtr(),
                dx.ToRawPtr(), nnz, N, N, 1.0, 0.0)
        _lib.check("CsrMV")
        return dy.to_numpy(), _info(cg.cusparse)[0]

    y5, c5 = product(_lib.COMPRESSION_PB)
    y4, c4 = product(_lib.COMPRESSION_BEST)
    assert (c5, c4) == (5, 4)
    assert np.array_equal(y5, ref) and np.array_equal(y4, y5)

    def solve(mode):
        L.MgcgSetMatrixCompression(cg.cusparse, mode)
        cg.x[:] = 0.0
        cg.vectorX.CopyFrom(cg.x, N)
        cg.Solve()
        cg.Read()
        assert _info(cg.cusparse)[0] == {1: 4, 3: 5}[mode]
        return cg.Iteration, cg.Residual, cg.x.copy()

    it5, res5, x5 = solve(_lib.COMPRESSION_PB)
    it4, res4, x4 = solve(_lib.COMPRESSION_BEST)
    assert res5 < 1e-8 and res4 < 1e-8 and abs(it5 - it4) <= 1
    assert np.abs(x5 - x4).max() <= 1e-8
    assert np.abs(x5 - (xs + 2.0)).max() <= 1e-7
    cg.Dispose()
