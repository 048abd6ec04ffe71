"""Multicolour ILU(0) on the GPU (MgSetupIlu0, ConjugateGradientIluGpu) against its numpy statement ``IluFactor`` in tests/test_ilu_host.py.

Everything is compared bit for bit: the five arrays of the factor, the pivot range, the colours and M^-1 r (whose sums are serial in every
mode); under dot_order = 1 SolveMg, SolveMinresMg, SolveBicgstabMg and SolveGmresMg are one fixed sequence of IEEE operations and must EQUAL
the numpy loops the other ...Mg suites compare against, with ``IluFactor.apply`` as M^-1.  Every refusal is checked for its message and for
the handle it must not leave."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.ilu import ConjugateGradientIluGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import same_bits, tuning
from tests.test_amg_host import csr_of, path_graph, serial_dot
from tests.test_bicgstab_host import MAX_IT
from tests.test_bicgstab_mg_host import level, pbicgstab_oracle
from tests.test_gmres_mg_host import fgmres_oracle
from tests.test_gpu_amg import _assert_same_solve, _maxnz, _solve
from tests.test_gpu_bicgstab_mg import assert_equal_runs, result_of as bicgstab_result
from tests.test_gpu_gmres_mg import finish as finish_gmres
from tests.test_gpu_pminres import _finish as finish_minres, assert_equal_runs as assert_equal_minres_runs
from tests.test_ilu_host import REFUSED, SHIFTS, SYSTEMS, IluFactor, IluLoop
from tests.test_pminres_host import m_norm, pminres_oracle

pytestmark = pytest.mark.gpu


def _ilu(s, shift=0.0, tol=1e-8, max_it=500, min_it=0):
    cg = ConjugateGradientIluGpu(s.Count, _maxnz(s), min_it, max_it, tol, shift=shift).load(s)
    cg.Initialize()
    return cg


def _assert_equals_the_yardstick(cg, F, what, seed=5):
    """The factor's five arrays, the pivot range, the colours and one application; returns what was read, for a second set-up to equal."""
    L = _lib.lib()
    assert L.MgIsIlu(cg.mg) == 1 and cg.levels == 1 and L.MgLevels(cg.mg) == 1 and L.MgLevelRows(cg.mg, 0) == F.n and L.MgLevelNnz(cg.mg, 0) == F.nnz
    e, c, ro, d, rowOf = cg.factor()
    assert same_bits(rowOf, F.rowOf.astype(np.int32)) and same_bits(ro, F.ro.astype(np.int32)), what
    assert same_bits(c, F.c.astype(np.int32)) and same_bits(d, F.diag.astype(np.int32)), what
    assert same_bits(e, F.e), what
    assert cg.colours() == F.colours() and cg.pivot_range() == F.pivot_range(), what
    r = np.random.default_rng(seed).standard_normal(F.n)
    zref = F.apply(r)
    z0 = cg.Apply(r)
    with tuning(dot_order=1):
        z1 = cg.Apply(r)
    assert same_bits(z0, zref) and same_bits(z1, zref), what
    return e, c, ro, d, rowOf, cg.pivot_range(), z0


def _same_reads(a, b):
    return all(same_bits(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))


# --------------------------------------------------------------------------- 1. set-up and one application = the yardstick
@functools.lru_cache(maxsize=None)
def _yardstick(name, shift):
    return IluFactor(*csr_of(SYSTEMS[name]()), shift=shift)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_setup_and_application_equal_the_yardstick_twice(name, shift):
    """The stencils in three stored orders (8 lanes a row), the band of 25 entries a row and the level of 46 rows and 26 colours (16 lanes,
    rows longer than a lane group), 1 to 5 rows (4 lanes)."""
    s, F = SYSTEMS[name](), _yardstick(name, shift)
    print(f"{name} shift {shift}: {F.n} rows, {F.nnz} entries, colours {F.colours()}, pivots {F.pivot_range()}")
    seen = []
    for _ in range(2):
        cg = _ilu(s, shift=shift)
        seen.append(_assert_equals_the_yardstick(cg, F, (name, shift)))
        cg.Dispose()
    assert _same_reads(*seen)


LANES = 2048 * 256                # kMaxGrid * kBlock of csrc/common.hpp: the lanes of one launch; a lane group is 4 of them on a path


def test_a_colour_longer_than_one_launch_takes_a_second_trip():
    """A path of 1.3 M rows: its first colour is a maximal independent set, about 0.43 of the rows -- more rows than one launch of the
    row-per-lane kernels has lanes, and more than four times what the lane-group kernels (build, factor, the two passes) hold."""
    s = path_graph(1300000, 5)
    F = IluFactor(*csr_of(s))
    assert int(np.diff(F.colourOffsets).max()) > LANES
    cg = _ilu(s)
    _assert_equals_the_yardstick(cg, F, "path of 1 300 000 rows")
    cg.Dispose()


# --------------------------------------------------------------------------- 2. the loops, bit for bit under dot_order = 1
def _poisson():
    return SYSTEMS["poisson6x5x4"]()


def _convdiff():
    s = SYSTEMS["convdiff6x5x4"]()
    s.b = np.random.default_rng(3).standard_normal(s.Count)
    return s


def test_solve_equals_the_numpy_pcg_loop():
    s = _poisson()
    ref = IluLoop(s).pcg(np.asarray(s.b), dot=serial_dot)
    plain = IluLoop(s)
    plain.apply = lambda r: r.copy()
    print(f"PCG: iterations {ref['iteration']}, plain CG {plain.pcg(np.asarray(s.b), dot=serial_dot)['iteration']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = _ilu(s)
        got = _solve(cg)
        cg.Dispose()
    _assert_same_solve(got, ref, "SolveMg with an ILU(0) handle")


@pytest.mark.parametrize("shift", [0.0, 5.0])
def test_minres_equals_its_numpy_loop(shift):
    """shift 5 lies inside the spectrum of the 6 x 5 x 4 Poisson matrix: A - 5 I is indefinite, M stays the factor of A."""
    s = _poisson()
    F = _yardstick("poisson6x5x4", 0.0)
    assert F.pivot_range()[0] > 0.0
    if shift:
        eig = np.linalg.eigvalsh(s.to_scipy().toarray())
        assert eig[0] < shift < eig[-1]
    tol = 1e-8 * m_norm(F.apply, np.asarray(s.b))
    ref = pminres_oracle(s, shift, F.apply, _lib.RULE_CSHARP, tol, max_it=3000)
    print(f"MINRES shift {shift}: iterations {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = _ilu(s, tol=tol, max_it=3000)
        got = finish_minres(cg, lambda: cg.SolveMinres(shift=shift, trace=True))
    assert_equal_minres_runs(got, ref)


@pytest.mark.parametrize("through", ["own", "hierarchy="])
def test_bicgstab_equals_its_numpy_loop(through):
    """"hierarchy=": the object's own factor is that of A + 0.1 D; the loop must run with the other object's factor of A."""
    s = _convdiff()
    a = s.to_scipy()
    assert (a != a.T).nnz > 0
    F = _yardstick("convdiff6x5x4", 0.0)
    ref = pbicgstab_oracle(s, F.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    print(f"BiCGStab: bodies {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = _ilu(s, tol=level(s), max_it=MAX_IT, shift=0.0 if through == "own" else 0.1)
        other = _ilu(s) if through != "own" else None
        try:
            cg.SolveBicgstab(trace=True, hierarchy=other)
        except ApplicationException:
            pass
        got = bicgstab_result(cg)
    cg.Dispose()
    if other is not None:
        other.Dispose()
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("through", ["own", "hierarchy="])
@pytest.mark.parametrize("orth", [1, 2])
def test_gmres_equals_its_numpy_loop(orth, through):
    s = _convdiff()
    F = _yardstick("convdiff6x5x4", 0.0)
    ref = fgmres_oracle(s, 9, orth, F.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    print(f"GMRES(9) orth {orth}: steps {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = _ilu(s, tol=level(s), max_it=MAX_IT, shift=0.0 if through == "own" else 0.1)
        other = _ilu(s) if through != "own" else None
        got = finish_gmres(cg, 9, orth, other)
    cg.Dispose()
    if other is not None:
        other.Dispose()
    assert_equal_runs(got, ref)


def test_an_ilu_object_preconditions_another_class_and_solves_poisson_with_gmres_too():
    """The handle of an ILU object behind an aggregation object's loop (hierarchy=), on the symmetric system."""
    s = _poisson()
    F = _yardstick("poisson6x5x4", 0.0)
    ref = fgmres_oracle(s, 9, 2, F.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, MAX_IT, level(s)).load(s)
        cg.Initialize()
        other = _ilu(s)
        got = finish_gmres(cg, 9, 2, other)
    cg.Dispose()
    other.Dispose()
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 3. refusals
def _system_of_arrays(e, c, ro, name):
    n = len(ro) - 1
    return problems.LinearSystem(np.ascontiguousarray(e, dtype=np.float64), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(ro, dtype=np.int32),
                                 np.zeros(n), np.ones(n), name)


@pytest.mark.parametrize("name", ["zero-pivot", "unsymmetric-pattern", "65-colours", "duplicate", "no-diagonal", "empty-row"])
def test_a_refused_matrix_leaves_no_handle_and_the_yardsticks_message(name):
    make, words = REFUSED[name]
    e, c, ro = make()
    with pytest.raises(ValueError) as err:
        IluFactor(e, c, ro)
    said = str(err.value)                                            # the yardstick names the row: the library must name the same one
    s = _system_of_arrays(e, c, ro, name)
    cg = ConjugateGradientIluGpu(s.Count, _maxnz(s), 0, 100, 1e-8).load(s)
    with pytest.raises(_lib.MgcgError) as refusal:
        cg.Initialize()
    msg = str(refusal.value)
    print(msg)
    assert "MgSetupIlu0: " in msg and said in msg, (said, msg)
    assert {"unsymmetric-pattern": "not structurally symmetric", "65-colours": "hold all 64 colours"}.get(name, words) in msg
    assert not cg.mg
    cg.Dispose()


def test_a_shifted_factor_exists_where_the_plain_one_is_refused():
    e, c, ro = REFUSED["zero-pivot"][0]()
    s = _system_of_arrays(e, c, ro, "ones")
    cg = _ilu(s, shift=0.5)
    _assert_equals_the_yardstick(cg, IluFactor(e, c, ro, shift=0.5), "ones, shift 0.5")
    cg.Dispose()


def test_a_handle_of_another_size_is_refused_by_the_solves():
    s, small = _poisson(), problems.poisson(6, 5, 2)
    cg, other = _ilu(s), _ilu(small)
    for run in (lambda: cg.SolveBicgstab(hierarchy=other), lambda: cg.SolveGmres(hierarchy=other, m=4)):
        with pytest.raises(_lib.MgcgError, match=f"the hierarchy has {small.Count} rows on level 0, the matrix has {s.Count}"):
            run()
    mine, cg.mg = cg.mg, other.mg
    try:
        with pytest.raises(_lib.MgcgError, match="hierarchy does not match the problem"):
            cg.Solve()
    finally:
        cg.mg = mine
    got = _solve(cg)                                                # the object still solves
    assert got["status"] == _lib.OK
    cg.Dispose()
    other.Dispose()


def test_the_hierarchy_calls_say_what_the_handle_is_and_a_second_setup_gives_the_same_bits():
    L = _lib.lib()
    s = SYSTEMS["poisson6x5x4-permuted"]()
    F = _yardstick("poisson6x5x4-permuted", 0.0)
    cg = _ilu(s)
    first = _assert_equals_the_yardstick(cg, F, "first set-up")
    out = np.zeros(s.Count, dtype=np.int32)
    calls = {"MgSetSmoother": lambda: L.MgSetSmoother(cg.mg, 1), "MgSetSmoother ": lambda: L.MgSetSmoother(cg.mg, 0),
             "MgSetInterpolation": lambda: L.MgSetInterpolation(cg.mg, 1), "MgLevelCopyAggregates": lambda: L.MgLevelCopyAggregates(cg.mg, 0, out.ctypes.data),
             "MgLevelCopyColours": lambda: L.MgLevelCopyColours(cg.mg, 0, out.ctypes.data)}
    for who, call in calls.items():
        L.MgcgClearLastError()
        assert call() == -1, who
        msg = _lib.last_error()
        L.MgcgClearLastError()
        assert msg.startswith(who.strip() + ": the handle is an ILU(0) factor (MgSetupIlu0)"), msg
    with pytest.raises(_lib.MgcgError, match="MgLevelCopyDinv: the handle is an ILU\\(0\\) factor"):
        cg.level_dinv(0)
    L.MgcgClearLastError()
    assert L.MgSetSmoother(cg.mg, 2) == -1 and "MgSetSmoother: mode 2, must be 0" in _lib.last_error()      # today's words
    L.MgcgClearLastError()
    assert L.MgSmoother(cg.mg) == 0 and L.MgLevelColours(cg.mg, 0) == 0
    assert _same_reads(first, _assert_equals_the_yardstick(cg, F, "after the refused calls"))
    # an aggregation hierarchy is no ILU handle
    amg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, 100, 1e-8).load(s)
    amg.Initialize()
    assert L.MgIsIlu(amg.mg) == 0 and L.MgIluColours(amg.mg) == -1 and "not an ILU(0) factor" in _lib.last_error()
    L.MgcgClearLastError()
    amg.Dispose()
    # MgDestroy and a new set-up on the same handles
    cg.Setup()
    assert _same_reads(first, _assert_equals_the_yardstick(cg, F, "second set-up"))
    cg.Dispose()
