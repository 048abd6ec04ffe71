"""Aggregation multigrid on the GPU (MgSetupAggregation / MgSetupAggregates) against its numpy statement in tests/test_amg_host.py and,
with 2x2x2 box aggregates, against the geometric hierarchy of MgSetup: maps, level matrices, D^-1 and the V-cycle are compared bit for
bit; the solves by iteration count and residual trace."""
import ctypes as C
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from tests.gpu_util import assert_trace_close, tuning
from tests.test_amg_host import Hierarchy, arrowhead, box_maps, csr_of, graph_laplacian, permuted, system_of

pytestmark = pytest.mark.gpu


def _maxnz(s):
    return int(np.diff(s.RowOffsets).max())


def _amg(s, tol=1e-8, max_it=500, **kw):
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, max_it, tol, **kw).load(s)
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


@functools.lru_cache(maxsize=None)
def _system(name):
    return SYSTEMS[name]()


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
