"""Aggregation multigrid on the GPU (MgSetupAggregation / MgSetupAggregates) against its numpy statement in tests/test_amg_host.py and,
with 2x2x2 box aggregates, against the geometric hierarchy of MgSetup: maps, level matrices, D^-1 and the V-cycle are compared bit for
bit; the solves by iteration count and residual trace and, under dot_order = 1, bit for bit with the yardstick's loop.

Sections 7 to 13 feed the kernels what the header's contract allows and a sorted symmetric grid matrix never shows them: rows in any
stored order, duplicate entries and stored zeros, entries without a mirror, the caller's aggregates of any size and numbering, levels
of one row and of more rows than one launch has lanes, bad diagonals on any level, and the solve with an initial guess, minIteration,
an iteration cap, every chunking, every compression mode and re-used level addresses."""
import ctypes as C
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from tests.gpu_util import assert_trace_close, cap_inside_a_chunk, same_bits, same_under_every_chunking, tuning
from tests.test_amg_host import (Hierarchy, arrowhead, box_maps, candidate_edges, csr_of, diagonal_first, dominant_graph, graph_laplacian, irregular_maps, one_way,
                                 pairs_with_a_negative_coarse_diagonal, path_graph, permuted, reversed_rows, rows_per_level, serial_dot, system_of,
                                 with_duplicates, zero_before_the_diagonal)

pytestmark = pytest.mark.gpu


def _maxnz(s):
    return int(np.diff(s.RowOffsets).max())


def _amg(s, tol=1e-8, max_it=500, min_it=0, x0=None, compression=None, **kw):
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), min_it, max_it, tol, **kw).load(s)
    if x0 is not None:
        cg.x[:] = x0
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    return cg


def _assert_apply_equals(cg, H, r, what):
    """M^-1 r against the yardstick.  The yardstick sums a matrix row in stored order; the library does so on every level whose rows hold
    20 entries or fewer on average, and sums longer rows by several lanes whose partial sums meet in a tree -- unless dot_order = 1
    (include/MgcgGpu.h: the validation mode, every sum in the reference's order).  So: EQUAL under dot_order = 1 on every system, and in
    the default mode within the rounding of a re-associated row sum.  That bound: a row of at most 330 products summed in another order
    moves by at most 330 * 2^-53 = 3.7e-14 of the sum of their magnitudes, the matrices here are diagonally dominant (that sum is at most
    twice |d x|), and a cycle of at most 8 levels, V(2,2) and 4 coarse sweeps chains fewer than 40 matrix passes none of which amplifies
    (omega D^-1 A has norm below 2): 40 * 2 * 3.7e-14 = 3e-12 of max |z|."""
    zref = H.apply(r)
    with tuning(dot_order=1):
        z1 = cg.Apply(r)
    z0 = cg.Apply(r)
    distance = float(np.abs(z0 - zref).max() / np.abs(zref).max())
    print(f"{what}: dot_order = 1 {'equal' if np.array_equal(z1, zref) else 'DIFFERENT'}; default mode max |z - yardstick| / max |yardstick| = {distance:.3e}, "
          f"{'equal' if np.array_equal(z0, zref) else 'not equal'} bit for bit")
    assert np.array_equal(z1, zref), what
    assert distance <= 3e-12, (what, distance)


def _assert_equal_hierarchies(cg, levels_of_reference):
    """cg's levels against a list of (e, c, ro, dinv)."""
    assert cg.levels == len(levels_of_reference)
    for l, (eo, co, ro, do) in enumerate(levels_of_reference):
        e, c, r = cg.level_csr(l)
        assert np.array_equal(r, ro) and np.array_equal(c, co) and np.array_equal(e, eo), l
        assert np.array_equal(cg.level_dinv(l), do), l


# --------------------------------------------------------------------------- 1. box aggregates = the geometric hierarchy
def _scaled(s, seed=4):
    """D A D of test_mg_variable_coefficients: SPD, the same pattern, varying values."""
    import scipy.sparse as sp

    d = sp.diags(1.0 + np.random.default_rng(seed).random(s.Count))
    out = system_of(d @ s.to_scipy() @ d, "scaled")
    out.grid = s.grid
    return out


@pytest.mark.parametrize("scaled", [False, True], ids=["poisson", "scaled"])
@pytest.mark.parametrize("dims", [(16, 16, 16), (8, 12, 4), (24, 16, 1)])
def test_box_aggregates_equal_the_geometric_hierarchy_bit_for_bit(dims, scaled):
    s = problems.poisson(*dims)
    if scaled:
        s = _scaled(s)
    r = np.random.default_rng(5).standard_normal(s.Count)
    for levels, nu, nuc in ((3, 1, 4), (2, 2, 3), (3, 3, 1)):
        geo = ConjugateGradientMgGpu(s.Count, 7, 0, 500, 1e-8, s.grid, levels=levels, nu=nu, nuCoarse=nuc).load(s)
        geo.Initialize()
        maps = box_maps(s.grid, levels)
        cg = _amg(s, omega=geo.omega, nu=nu, nuCoarse=nuc, aggregates=maps)
        assert geo.levels == len(maps) + 1
        _assert_equal_hierarchies(cg, [geo.level_csr(l) + (geo.level_dinv(l),) for l in range(geo.levels)])
        for l, m in enumerate(maps):
            assert np.array_equal(cg.level_aggregates(l), m)
        assert np.array_equal(cg.Apply(r), geo.Apply(r)), (dims, scaled, levels, nu, nuc)
        cg.Dispose()
        geo.Dispose()


# --------------------------------------------------------------------------- 2. the library's aggregates = the yardstick
SYSTEMS = {
    "poisson12-permuted": lambda: permuted(problems.poisson(12, 12, 12), 7),          # 1 728 rows
    "random_spd3000": lambda: problems.random_spd(3000),
    "graph10": lambda: graph_laplacian(10, 3),                                        # 1 000 rows, weights 10^U(0,3), + 1e-3 I
    "arrowhead1037": arrowhead,                                                       # one row of 322 negative entries
}


# Stored order: rows that are not sorted, hold duplicate entries and explicit zeros, or have no mirror entry.  Every one is a diagonally
# dominant M-matrix (a row keeps its entries' magnitudes, in another order or split 1 : 3; a one-way entry raises its row's diagonal by its
# own size) of at most 14 entries a row, on at most 8 levels: the premises of _assert_apply_equals' default-mode bound hold.
STORED_ORDER = {
    "reversed": lambda: reversed_rows(_system("poisson12-permuted")),
    "diagonal-first": lambda: diagonal_first(_system("poisson12-permuted")),
    "duplicates": lambda: with_duplicates(graph_laplacian(8, 3)),                     # 512 rows, 2 x the entries
    "one-way": lambda: one_way(_system("graph10")),                                   # 150 entries without a mirror
}


@functools.lru_cache(maxsize=None)
def _system(name):
    return {**SYSTEMS, **STORED_ORDER}[name]()


@functools.lru_cache(maxsize=None)
def _yardstick(name, passes):
    return Hierarchy(*csr_of(_system(name)), passes=passes)           # the defaults of ConjugateGradientAmgGpu


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_library_aggregates_equal_the_yardstick(name, passes, nu):
    s = _system(name)
    H = _yardstick(name, passes)
    H.nu = nu
    cg = _amg(s, passes=passes, nu=nu)
    print(f"{name}: rows per level {[len(L['ro']) - 1 for L in H.levels]}")
    assert len(H.levels) >= 2, "the case must coarsen to test anything"
    _assert_equal_hierarchies(cg, [(L["e"], L["c"], L["ro"], L["dinv"]) for L in H.levels])
    for l, L in enumerate(H.levels[:-1]):
        assert np.array_equal(cg.level_aggregates(l), L["map"]), l
    _assert_apply_equals(cg, H, np.random.default_rng(5).standard_normal(s.Count), f"{name} passes {passes} nu {nu}")
    cg.Dispose()


# --------------------------------------------------------------------------- 3. properties
def test_preconditioner_is_symmetric_and_cuts_iterations_on_a_permuted_grid():
    s = permuted(problems.poisson(32, 32, 32), 11)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    cg = _amg(s, levels=3, omega=6.0 / 7.0)
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal(s.Count), rng.standard_normal(s.Count)
    a, b = float(u @ cg.Apply(v)), float(v @ cg.Apply(u))
    assert abs(a - b) <= 1e-12 * abs(a)
    H = Hierarchy(*csr_of(s), levels=3, omega=6.0 / 7.0)
    ref = H.pcg(np.asarray(s.b), tol=1e-8)
    cg.Solve(trace=True)
    cg.Read()
    plain = ConjugateGradientSingleGpu(s.Count, 7, 0, 2000, 1e-8, rule=_lib.RULE_CSHARP).load(s)
    plain.Initialize()
    plain.Solve()
    print(f"rows per level {[len(L['ro']) - 1 for L in H.levels]}, iterations: V-cycle {cg.Iteration}, yardstick {ref['iteration']}, SolveEx {plain.Iteration}")
    assert cg.levels == 3
    assert cg.Iteration == ref["iteration"]
    assert_trace_close(cg.trace, ref["trace"])
    assert 3 * cg.Iteration < plain.Iteration
    assert np.linalg.norm(s.b - s.to_scipy() @ cg.x) < 2e-8
    plain.Dispose()
    cg.Dispose()


def test_jumping_coefficients_need_fewer_iterations_than_jacobi():
    s = graph_laplacian(20, 3)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    cg = _amg(s, tol=tol, max_it=2000, levels=3, omega=6.0 / 7.0)
    cg.Solve()
    cg.Read()
    jac = ConjugateGradientJacobiGpu(s.Count, _maxnz(s), 0, 2000, tol, rule=_lib.RULE_CSHARP).load(s)
    jac.Initialize()
    jac.Solve()
    print(f"iterations: V-cycle {cg.Iteration}, SolveJacobi {jac.Iteration}")
    assert cg.Iteration < jac.Iteration
    assert np.linalg.norm(s.b - s.to_scipy() @ cg.x) < 2.0 * tol
    jac.Dispose()
    cg.Dispose()


# --------------------------------------------------------------------------- 4. no coupling
def test_a_matrix_without_couplings_gives_one_level_of_jacobi_sweeps():
    s = problems.viennacl_main(n=2000)
    H = Hierarchy(*csr_of(s))
    if len(H.levels) != 1:
        pytest.fail("the yardstick matches rows of this matrix: the case no longer tests what it is for")
    cg = _amg(s, max_it=2000)
    assert cg.levels == 1 and _lib.lib().MgLevels(cg.mg) == 1
    _assert_apply_equals(cg, H, np.random.default_rng(5).standard_normal(s.Count), "viennacl_main(2000)")     # nuCoarse Jacobi sweeps
    with pytest.raises(_lib.MgcgError, match="no map"):
        cg.level_aggregates(0)
    cg.Solve()
    cg.Read()
    assert cg.status == _lib.OK and np.linalg.norm(s.b - s.to_scipy() @ cg.x) < 2e-8
    cg.Dispose()


# --------------------------------------------------------------------------- 5. refusals
def test_refusals_carry_a_message(mgcg_env):
    L = _lib.lib()
    s = problems.poisson(8, 8, 4)
    # a row without a stored diagonal
    keep = np.ones(s.nnz, dtype=bool)
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    keep[np.nonzero((rows == 37) & (np.asarray(s.ColumnIndeces[: s.nnz]) == 37))[0]] = False
    ro = np.r_[0, np.cumsum(np.bincount(rows[keep], minlength=s.Count))].astype(np.int32)
    holed = problems.LinearSystem(s.Elements[: s.nnz][keep], s.ColumnIndeces[: s.nnz][keep], ro, s.x, s.b, "no-diagonal")
    for kw in (dict(), dict(aggregates=box_maps(s.grid, 2))):
        with pytest.raises(_lib.MgcgError, match="level 0, row 37: the diagonal"):
            _amg(holed, **kw)
    # the caller's maps: an id out of range, an empty aggregate
    m0, m1 = box_maps(s.grid, 3)
    bad = m0.copy()
    bad[5] = len(m1)
    with pytest.raises(_lib.MgcgError, match=f"level 0, row 5: aggregate id {len(m1)} out of range"):
        _amg(s, aggregates=[bad, m1])
    bad = m0.copy()
    bad[bad == 3] = 2
    with pytest.raises(_lib.MgcgError, match="level 0: aggregate 3 is empty"):
        _amg(s, aggregates=[bad, m1])
    # the linear transfer needs a grid; a geometric hierarchy has no stored maps
    cg = _amg(s, levels=3)
    L.MgcgClearLastError()
    assert L.MgSetInterpolation(cg.mg, 1) == -1 and "needs a grid" in _lib.last_error()
    L.MgcgClearLastError()
    assert L.MgSetInterpolation(cg.mg, 0) == 0
    geo = ConjugateGradientMgGpu(s.Count, 7, 0, 500, 1e-8, s.grid).load(s)
    geo.Initialize()
    out = np.zeros(s.Count, dtype=np.int32)
    assert L.MgLevelCopyAggregates(geo.mg, 0, out.ctypes.data) == -1 and "geometric hierarchy" in _lib.last_error()
    L.MgcgClearLastError()
    assert L.MgLevelCopyAggregates(cg.mg, cg.levels - 1, out.ctypes.data) == -1 and "no map" in _lib.last_error()
    L.MgcgClearLastError()
    geo.Dispose()
    cg.Dispose()
    # two loopback ranks: the hierarchy is one rank's, SolveMgParallel says so on both
    from tests.test_gpu_jacobi import run_ranks

    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", "2")

    def make_rank(rank, comm):
        one = _amg(s, levels=3)
        it, res = C.c_int(0), C.c_double(0.0)
        L.MgcgClearLastError()
        st = L.SolveMgParallel(comm, one.cublas, one.cusparse, one.matDescr, one.mg, one.vectorA.Ptr, one.vectorRowOffsets.Ptr, one.vectorColumnIndeces.Ptr,
                               one.vectorX.Ptr, one.vectorB.Ptr, one.vectorAp.Ptr, one.vectorP.Ptr, one.vectorR.Ptr, one.vectorZ.Ptr,
                               s.Count, s.Count, 0, s.nnz, 0, s.Count - 1, 1e-8, 0, 500, _lib.RULE_CSHARP, C.byref(it), C.byref(res), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        one.Dispose()
        return st, msg

    for st, msg in run_ranks(2, make_rank, timeout=120):
        assert st == _lib.ERROR and "the hierarchy was built for 1 rank(s)" in msg, (st, msg)


# --------------------------------------------------------------------------- 6. determinism
def test_two_setups_give_the_same_maps_and_the_same_bits():
    s = _system("random_spd3000")
    r = np.random.default_rng(5).standard_normal(s.Count)
    runs = []
    for _ in range(2):
        cg = _amg(s)
        runs.append(([cg.level_aggregates(l) for l in range(cg.levels - 1)], cg.Apply(r)))
        cg.Dispose()
    assert len(runs[0][0]) == len(runs[1][0]) >= 1
    assert all(np.array_equal(p, q) for p, q in zip(runs[0][0], runs[1][0]))
    assert runs[0][1].tobytes() == runs[1][1].tobytes()
    # ... and a solve on the hierarchy converges
    cg = _amg(s)
    try:
        cg.Solve()
    except ApplicationException:
        pytest.fail("SolveMg did not converge on random_spd(3000)")
    cg.Read()
    assert np.linalg.norm(s.b - s.to_scipy() @ cg.x) < 2e-8
    cg.Dispose()


# --------------------------------------------------------------------------- 7. stored order
def _levels_of(H):
    return [(L["e"], L["c"], L["ro"], L["dinv"]) for L in H.levels]


def _assert_equals_the_yardstick(cg, H, what, seed=5):
    """The file's comparison: CSR, offsets and D^-1 of every level, every map, M^-1 r."""
    print(f"{what}: rows per level {rows_per_level(H)}")
    _assert_equal_hierarchies(cg, _levels_of(H))
    for l, L in enumerate(H.levels[:-1]):
        assert np.array_equal(cg.level_aggregates(l), L["map"]), l
    _assert_apply_equals(cg, H, np.random.default_rng(seed).standard_normal(len(H.levels[0]["ro"]) - 1), what)


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("name", list(STORED_ORDER))
def test_rows_in_any_stored_order_equal_the_yardstick(name, passes, nu):
    """The contract speaks of stored order: the diagonal is the first stored entry of column i wherever it stands, the Galerkin sum takes
    a member's entries as stored, duplicates are separate entries; "one-way" ends its first pass by the round that pairs nobody."""
    s = _system(name)
    H = _yardstick(name, passes)
    H.nu = nu
    assert len(H.levels) >= 2, "the case must coarsen to test anything"
    cg = _amg(s, passes=passes, nu=nu)
    _assert_equals_the_yardstick(cg, H, f"{name} passes {passes} nu {nu}")
    cg.Dispose()


# --------------------------------------------------------------------------- 8. the caller's maps, of any size and numbering
@functools.lru_cache(maxsize=None)
def _irregular():
    """dominant_graph(10, 3) under irregular_maps: aggregates of 1 .. 40 scattered rows, ids in no order, then % 5, then one aggregate.
    A strictly dominant M-matrix and its Galerkin products (dominant M-matrices again), 4 levels, rows of at most 1000 / 40 < 330 entries:
    the premises of the default-mode bound hold; level 1 holds more than 20 entries a row, so the default mode sums its rows by lanes."""
    s = dominant_graph(10, 3)
    maps = irregular_maps(s.Count)
    return s, maps, Hierarchy(*csr_of(s), maps=maps)


def test_irregular_aggregates_of_the_caller_equal_the_yardstick():
    s, maps, H = _irregular()
    assert rows_per_level(H) == [1000, len(maps[1]), 5, 1] and len(H.levels[1]["e"]) > 20 * len(maps[1])
    for nu in (1, 2):
        H.nu = nu
        cg = _amg(s, nu=nu, aggregates=maps)
        assert cg.levels == 4
        for l, m in enumerate(maps):
            assert same_bits(cg.level_aggregates(l), m), l                # what was passed, not a renumbering
        _assert_equals_the_yardstick(cg, H, f"irregular maps nu {nu}")
        cg.Dispose()
    H.nu = 1


def test_the_identity_map_with_sigma_1_reproduces_the_matrix():
    s = _system("arrowhead1037")
    e, c, ro = csr_of(s)
    cg = _amg(s, sigma=1.0, aggregates=[np.arange(s.Count, dtype=np.int32)])
    assert cg.levels == 2
    assert same_bits(cg.level_csr(1), (e, c.astype(np.int32), ro.astype(np.int32)))
    assert same_bits(cg.level_dinv(1), cg.level_dinv(0))
    cg.Dispose()


def test_no_map_at_all_gives_one_level_of_jacobi_sweeps():
    s = _irregular()[0]
    for sweeps in (1, 4):
        H = Hierarchy(*csr_of(s), nuCoarse=sweeps, maps=[])
        cg = _amg(s, nuCoarse=sweeps, aggregates=[])
        assert cg.levels == 1 == len(H.levels)
        _assert_equals_the_yardstick(cg, H, f"aggregates=[] with {sweeps} sweeps")       # (a strictly dominant M-matrix of 7 entries a row)
        if sweeps == 1:
            r = np.random.default_rng(6).standard_normal(s.Count)
            assert same_bits(cg.Apply(r), 0.8 * (H.levels[0]["dinv"] * r))
        cg.Dispose()


# --------------------------------------------------------------------------- 9. tiny matrices
def _solve(cg, trace=True):
    """SolveMg -> dict(status, iteration, residual, trace, x); the cap is a result here, not an exception."""
    try:
        cg.Solve(trace=trace)
    except ApplicationException:
        assert cg.status == _lib.MAXIT_EXCEEDED
    cg.Read()
    return dict(status=cg.status, iteration=cg.Iteration, residual=cg.Residual, trace=cg.trace.copy(), x=cg.x.copy())


def _assert_same_solve(got, ref, what):
    assert (got["status"], got["iteration"]) == (ref["status"], ref["iteration"]), (what, got["status"], got["iteration"], ref["status"], ref["iteration"])
    assert same_bits(got["trace"], ref["trace"]), what
    assert got["residual"] == ref["residual"], what
    assert same_bits(got["x"], ref["x"]), what


@pytest.mark.parametrize("n,rows", [(1, [1]), (2, [2, 1]), (3, [3, 1]), (5, [5, 1])])
def test_tiny_matrices_set_up_apply_and_solve(n, rows):
    """The 1-D Laplacian (diagonal 4: strictly dominant, 3 entries a row, at most 2 levels) down to a single row."""
    s = problems.poisson(n, 1, 1)
    H = Hierarchy(*csr_of(s), minCoarse=0)
    assert rows_per_level(H) == rows
    cg = _amg(s, minCoarse=0)
    _assert_equals_the_yardstick(cg, H, f"{n} row(s)")
    with tuning(dot_order=1):
        got = _solve(cg)
    assert got["status"] == _lib.OK and np.linalg.norm(s.b - s.to_scipy() @ got["x"]) < 2e-8
    _assert_same_solve(got, H.pcg(np.asarray(s.b), dot=serial_dot), f"{n} row(s)")
    cg.Dispose()


# --------------------------------------------------------------------------- 10. beyond one grid of lanes
LANES = 2048 * 256                # kMaxGrid * kBlock of csrc/common.hpp: the lanes of one launch of kernels_amg.hip; more rows mean a second trip


@functools.lru_cache(maxsize=None)
def _long_path(kind):
    if kind == "uniform":
        s = path_graph(2 * LANES + 1077, 5)
        return s, Hierarchy(*csr_of(s), levels=3, passes=1)
    s = path_graph(LANES + 1077, 5, decades=2.0)
    return s, Hierarchy(*csr_of(s), levels=2, passes=1)


@pytest.mark.parametrize("kind", ["uniform", "wide"])
def test_every_stride_loop_takes_a_second_trip(kind):
    """uniform: a path of 1 049 653 rows, one pass a level: fine AND coarse rows of the first Galerkin product exceed the lanes of a launch,
    so pick, match, count, fill, diagonal check, restriction and prolongation all come round again.  Its weights U(0.5, 2) all pass the
    threshold 0.25 whatever the row maxima are, so `wide` (525 365 rows, weights over two decades more) has the threshold decide: the
    map then needs the row maximum of the rows of the second trip.  Strictly dominant, 3 entries a row, at most 3 levels: the premises
    of the default-mode bound hold."""
    s, H = _long_path(kind)
    rows = rows_per_level(H)
    if kind == "wide":
        e, c, ro = csr_of(s)
        assert rows[0] > LANES and len(rows) == 2 and len(candidate_edges(e, c, ro, 0.25)[0]) < 0.9 * (s.nnz - s.Count), rows
        cg = _amg(s, levels=2, passes=1)
        _assert_equals_the_yardstick(cg, H, "path of 2048 * 256 + 1077 rows, weights over 2.6 decades")
        cg.Dispose()
        return
    assert len(rows) == 3 and rows[0] > 2 * LANES and rows[1] > LANES, rows
    cg = _amg(s, levels=3, passes=1)
    _assert_equals_the_yardstick(cg, H, "path of 2 * 2048 * 256 + 1077 rows")
    # ... and the diagonal check reaches the rows of its second trip: the same handles refuse a bad row there, before anything is built
    bad = s.Count - 5
    cg.load(_with_diagonal(s, bad, -1.0))
    with pytest.raises(_lib.MgcgError, match=f"level 0, row {bad}: the diagonal"):
        cg.Initialize()
    cg.Dispose()


# --------------------------------------------------------------------------- 11. refusals on any level, and the handles afterwards
def _with_diagonal(s, where, value):
    """s with the diagonal entries of the rows `where` set to `value`."""
    out = problems.LinearSystem(np.array(s.Elements[: s.nnz], dtype=np.float64), s.ColumnIndeces[: s.nnz].copy(), s.RowOffsets.copy(), s.x.copy(), s.b.copy(), s.name)
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    out.Elements[np.isin(rows, where) & (out.ColumnIndeces == rows)] = value
    return out


@functools.lru_cache(maxsize=None)
def _refusal_base(entry):
    """(good system, keywords, its yardstick) of the two entry points: the library's matching, the caller's boxes."""
    s = problems.poisson(8, 8, 4)
    kw = dict() if entry == "matching" else dict(aggregates=box_maps(s.grid, 2))
    return s, kw, Hierarchy(*csr_of(s), maps=kw.get("aggregates"))


def _refused_then_built(bad, good, H, message, **kw):
    """One set of handles: the bad matrix is refused with `message`, then the good one is set up and equals its yardstick -- the
    half-built hierarchy was freed and left nothing behind."""
    cg = ConjugateGradientAmgGpu(good.Count, max(_maxnz(bad), _maxnz(good)), 0, 500, 1e-8, **kw).load(bad)
    with pytest.raises(_lib.MgcgError, match=message):
        cg.Initialize()
    assert not cg.mg
    cg.load(good)
    cg.Initialize()
    _assert_equals_the_yardstick(cg, H, f"after the refusal '{message}'")       # (the dominant 7-point stencil / its good-pairs twin)
    cg.Dispose()


@pytest.mark.parametrize("entry", ["matching", "boxes"])
@pytest.mark.parametrize("kind", ["zero-first", "negative", "nan", "infinite"])
def test_a_bad_diagonal_on_level_0_is_refused_and_the_handles_stay_usable(kind, entry):
    s, kw, H = _refusal_base(entry)
    bad = zero_before_the_diagonal(s, 37) if kind == "zero-first" else _with_diagonal(s, 37, {"negative": -6.0, "nan": np.nan, "infinite": np.inf}[kind])
    _refused_then_built(bad, s, H, "level 0, row 37: the diagonal", **kw)


@pytest.mark.parametrize("entry", ["matching", "pairs"])
def test_a_bad_diagonal_made_by_the_galerkin_sum_is_refused_and_the_handles_stay_usable(entry):
    """100 blocks [[1, -2], [-2, 1]]: level 0 passes, level 1's diagonal is sigma (1 - 2 - 2 + 1) < 0.  The good twin has 3 on the diagonal."""
    bad = pairs_with_a_negative_coarse_diagonal()
    good = _with_diagonal(bad, np.arange(200), 3.0)
    kw = dict() if entry == "matching" else dict(aggregates=[np.arange(200, dtype=np.int32) // 2])
    H = Hierarchy(*csr_of(good), maps=kw.get("aggregates"))
    assert rows_per_level(H) == [200, 100]
    _refused_then_built(bad, good, H, "level 1, row 0: the diagonal", **kw)


# --------------------------------------------------------------------------- 12. SolveMg on an aggregation hierarchy, bit for bit
@functools.lru_cache(maxsize=None)
def _solve_case(name):
    """(system, constructor keywords, yardstick) of the four hierarchies of the solve tests."""
    if name == "irregular":
        s, maps, H = _irregular()
        return s, dict(aggregates=maps), H
    if name == "one-level":                       # no negative coupling: the finest level is the coarsest, r.z rides on its last sweep
        s = problems.viennacl_main(n=2000)
        H = Hierarchy(*csr_of(s))
        assert len(H.levels) == 1
        return s, dict(), H
    return _system(name), dict(), _yardstick(name, 3)


@functools.lru_cache(maxsize=None)
def _reference_solve(name, variant):
    s, _, H = _solve_case(name)
    H.nu = 1
    b = np.asarray(s.b)
    free = H.pcg(b, dot=serial_dot)
    if variant == "plain":
        return dict(), free
    if variant == "guess":
        x0 = np.random.default_rng(8).standard_normal(s.Count)
        return dict(x0=x0), H.pcg(b, x0=x0, dot=serial_dot)
    if variant == "min-iteration":
        min_it = free["iteration"] + 4
        return dict(min_it=min_it), H.pcg(b, dot=serial_dot, min_it=min_it)
    cap = cap_inside_a_chunk(0, free["iteration"])
    return dict(max_it=cap), H.pcg(b, dot=serial_dot, max_it=cap)


@pytest.mark.parametrize("variant", ["plain", "guess", "min-iteration", "cap"])
@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10", "irregular", "one-level"])
def test_solve_equals_the_yardstick_loop_bit_for_bit(name, variant):
    """dot_order = 1: trace, iteration, residual and x of SolveMg equal Hierarchy.pcg with serial dots (which IS oracle_pcg: test_amg_host)."""
    s, kw, _ = _solve_case(name)
    how, ref = _reference_solve(name, variant)
    print(f"{name} {variant}: yardstick iteration {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == (_lib.MAXIT_EXCEEDED if variant == "cap" else _lib.OK)
    if variant == "min-iteration":
        assert ref["iteration"] == how["min_it"] and ref["trace"][-5] < 1e-8          # it ran on past convergence
    if variant == "cap":
        assert ref["iteration"] == how["max_it"] + 1 and ref["residual"] > 1e-8
    with tuning(dot_order=1):
        cg = _amg(s, **how, **kw)
        got = _solve(cg)
        cg.Dispose()
    _assert_same_solve(got, ref, (name, variant))


@pytest.mark.parametrize("order", [0, 1])
def test_chunking_cannot_change_a_solve(order):
    """check_every = 1, 4, 7: the same bits, also when the iteration cap ends the loop in the middle of a chunk."""
    s, kw, _ = _solve_case("graph10")

    def run(max_it):
        cg = _amg(s, max_it=max_it, **kw)
        out = _solve(cg)
        cg.Dispose()
        return out

    free = same_under_every_chunking(lambda: run(500), order)
    assert free["status"] == _lib.OK and free["iteration"] > 8
    cap = cap_inside_a_chunk(0, free["iteration"])
    capped = same_under_every_chunking(lambda: run(cap), order)
    print("iteration", free["iteration"], "cap", cap)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == cap + 1
    if order == 1:
        _assert_same_solve(free, _reference_solve("graph10", "plain")[1], "check_every")
        _assert_same_solve(capped, _reference_solve("graph10", "cap")[1], "check_every, capped")


# --------------------------------------------------------------------------- 13. compression modes and address reuse
def _classes(cg):
    """The class of every analysis the handle holds (MgcgAnalysisInfo): 0 = plain CSR kept, 1 .. 5 = a lossless form in use."""
    L, out = _lib.lib(), []
    while L.MgcgAnalysisInfo(cg.cusparse, len(out), None, None, None, None) >= 0:
        out.append(L.MgcgAnalysisInfo(cg.cusparse, len(out), None, None, None, None))
    return out


def _everything(cg, s):
    """Set-up bits, M^-1 r and the solve of one hierarchy under dot_order = 1."""
    out = dict(classes=_classes(cg), levels=[cg.level_csr(l) + (cg.level_dinv(l),) for l in range(cg.levels)], maps=[cg.level_aggregates(l) for l in range(cg.levels - 1)])
    with tuning(dot_order=1):
        out["apply"] = cg.Apply(np.random.default_rng(5).standard_normal(s.Count))
        out["solve"] = _solve(cg)
    return out


@functools.lru_cache(maxsize=None)
def _plain_form(name):
    s = _system(name)
    cg = _amg(s, compression=0)
    out = _everything(cg, s)
    cg.Dispose()
    return out


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10"])
def test_matrix_compression_changes_no_bit(name, mode):
    """The lossless forms of MgcgSetMatrixCompression on every level's matrix: the set-up is the same bits in every mode, and under
    dot_order = 1 so are M^-1 r and the solve; both equal the yardstick."""
    s = _system(name)
    plain = _plain_form(name)
    cg = _amg(s, compression=mode)
    got = _everything(cg, s)
    cg.Dispose()
    print(f"{name} mode {mode}: analysis classes {got['classes']}, mode 0 {plain['classes']}")
    assert len(got["levels"]) == len(plain["levels"]) >= 2 and not any(plain["classes"])
    if name == "graph10":                         # sorted rows of a grid graph, 7 distinct offsets: one byte per nonzero in every mode
        assert max(got["classes"]) >= 1, "no level took a compressed form: the case tests nothing"
    assert same_bits(got["levels"], plain["levels"]) and same_bits(got["maps"], plain["maps"])
    assert same_bits(got["apply"], plain["apply"])
    H = _yardstick(name, 3)
    H.nu = 1
    assert same_bits(got["apply"], H.apply(np.random.default_rng(5).standard_normal(s.Count)))
    for key in ("status", "iteration", "residual"):
        assert got["solve"][key] == plain["solve"][key], key
    assert same_bits(got["solve"]["trace"], plain["solve"]["trace"]) and same_bits(got["solve"]["x"], plain["solve"]["x"])
    _assert_same_solve(got["solve"], _reference_solve(name, "plain")[1], (name, mode))


def test_a_rebuilt_hierarchy_is_analysed_afresh():
    """MgDestroy frees the level arrays and the next set-up may be handed the same addresses: with the analysis cache on (mode 1), a
    hierarchy built on the same handles for a matrix of the same pattern and other values must be its own matrix's, twice over."""
    a = problems.poisson(16, 16, 16)
    b = _scaled(a)
    maps = box_maps(a.grid, 3)
    H = {id(m): Hierarchy(*csr_of(m), omega=6.0 / 7.0, maps=maps) for m in (a, b)}
    assert not np.array_equal(H[id(a)].levels[1]["e"], H[id(b)].levels[1]["e"]) and np.array_equal(H[id(a)].levels[1]["c"], H[id(b)].levels[1]["c"])
    cg = ConjugateGradientAmgGpu(a.Count, 7, 0, 500, 1e-8, omega=6.0 / 7.0, aggregates=maps)
    _lib.lib().MgcgSetMatrixCompression(cg.cusparse, 1)
    for turn, m in enumerate((a, b, a, b)):
        cg.load(m)
        cg.Initialize()
        # (7 entries a row on every level: both modes sum every row in stored order, the default-mode distance is 0 by construction)
        _assert_equals_the_yardstick(cg, H[id(m)], f"turn {turn}")
        assert max(_classes(cg)) >= 1, "no level took a compressed form: there is no analysis that could be stale"
        _lib.lib().MgDestroy(cg.mg)
        cg.mg = None
    cg.Dispose()
    # ... and with the library's own aggregates, whose passes allocate and free intermediate matrices as well
    a, b = _system("graph10"), graph_laplacian(10, 4)                    # the same grid graph, other weights: dominant M-matrices both
    assert np.array_equal(a.ColumnIndeces, b.ColumnIndeces) and not np.array_equal(a.Elements, b.Elements)
    cg = ConjugateGradientAmgGpu(a.Count, _maxnz(a), 0, 500, 1e-8)
    _lib.lib().MgcgSetMatrixCompression(cg.cusparse, 1)
    for turn, m in enumerate((a, b, a, b)):
        cg.load(m)
        cg.Initialize()
        Hm = _yardstick("graph10", 3) if m is a else Hierarchy(*csr_of(m))
        Hm.nu = 1
        _assert_equals_the_yardstick(cg, Hm, f"graph10, turn {turn}")
        _lib.lib().MgDestroy(cg.mg)
        cg.mg = None
    cg.Dispose()
