"""LOBPCG on the GPU (MgcgSolveLobpcg, MgcgSolveLobpcgMg, eigen.SymmetricEigenGpu and SolveLobpcg of the hierarchy classes).

The reference for every comparison is ``lobpcg_oracle`` (tests/test_lobpcg_host.py): the header's loop in numpy with serial sums.  Under
dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, restarts, theta, the residuals, the true
residuals, the trace and ALL of X must EQUAL it; in the default mode only the summation order of the Gram entries differs, and the
device's own results must keep the four promises of the host file with a body count within 2 of the oracle's."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.eigen import SymmetricEigenGpu
from conjugategradient_amd.ilu import ConjugateGradientIluGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException
from conjugategradient_amd.ssor import ConjugateGradientSsorGpu
from tests.test_amg_host import Hierarchy, box_maps, csr_of, permuted
from tests.test_bicgstab_mg_host import class_omega
from tests.test_gs_host import GsHierarchy
from tests.test_ilu_host import IluFactor
from tests.test_lobpcg_host import BODY_COUNT_UNSTABLE, EPS, check_promises, diagonal_system, lobpcg_oracle, reference, start_block, system

pytestmark = pytest.mark.gpu

TOL = 1e-8
W_BREAKDOWN = "the factorisation of W^T W (a zero or dependent column of W)"
START_BREAKDOWN = "the first factorisation, of X0^T X0 (dependent or zero start columns)"


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def _maxnz(s):
    return max(int(np.diff(s.RowOffsets).max()), 1)


def result_of(cg, message=""):
    return dict(status=cg.status, column_status=[int(v) for v in cg.ColumnStatus], iteration=cg.Iteration, restarts=cg.Restarts, theta=cg.Theta.copy(),
                residual=cg.Residual.copy(), true_residual=cg.TrueResidual.copy(), trace=cg.trace, X=cg.X, message=message)


def run(cg, solve):
    """One solve; an iteration cap that was hit or a breakdown is a result here, not an exception."""
    message = ""
    try:
        solve()
    except ApplicationException:
        assert cg.status == _lib.MAXIT_EXCEEDED
    except _lib.MgcgError as e:
        assert cg.status == _lib.NONFINITE
        message = str(e)
    return result_of(cg, message)


def solve(s, k, tol=TOL, relative=True, largest=False, jacobi=False, X0=None, seed=1, min_it=0, max_it=1000, compression=None, trace_capacity=None):
    cg = SymmetricEigenGpu(s.Count, _maxnz(s), k, min_it, max_it, tol, relative=relative, largest=largest, jacobi=jacobi).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    out = run(cg, lambda: cg.Solve(trace=True, X0=X0, seed=seed, traceCapacity=trace_capacity))
    cg.Dispose()
    return out


def assert_equal_runs(got, ref, trace_rows=None):
    assert got["status"] == ref["status"], (got["status"], ref["status"], got["message"])
    assert got["column_status"] == ref["column_status"]
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert got["restarts"] == ref["restarts"], (got["restarts"], ref["restarts"])
    for key in ("theta", "residual", "true_residual", "X"):
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    rows = len(ref["trace"]) if trace_rows is None else trace_rows
    assert np.array_equal(got["trace"], ref["trace"][:rows], equal_nan=True)


# --------------------------------------------------------------------------- 1. bit equality with the oracle
EQUAL = [("poisson765", k, jacobi, False) for k in (1, 2, 3, 5, 8) for jacobi in (False, True)] + [("spd600", 4, True, False), ("poisson765", 2, False, True)]


@pytest.mark.parametrize("name,k,jacobi,largest", EQUAL)
def test_solve_equals_the_oracle_bit_for_bit(dot_order, name, k, jacobi, largest):
    ref = reference(name, k, jacobi=jacobi, largest=largest)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    got = solve(system(name), k, jacobi=jacobi, largest=largest)
    print(name, k, jacobi, largest, "bodies", got["iteration"], ref["iteration"], "restarts", got["restarts"], ref["restarts"], "theta", got["theta"])
    assert_equal_runs(got, ref)


def within_two_bodies(got, ref):
    print("bodies", got["iteration"], "oracle", ref["iteration"])
    assert abs(got["iteration"] - ref["iteration"]) <= 2, (got["iteration"], ref["iteration"])


@pytest.mark.parametrize("name,k,jacobi,largest", EQUAL)
def test_default_mode_keeps_the_promises(name, k, jacobi, largest):
    """The four promises on every case; the body count within 2 of the oracle's on the cases on which the oracle itself stays within 2
    when only the order of its Gram sums changes (tests/test_lobpcg_host.py: BODY_COUNT_UNSTABLE has the others and their figures)."""
    ref = reference(name, k, jacobi=jacobi, largest=largest)
    got = solve(system(name), k, jacobi=jacobi, largest=largest)
    check_promises(system(name), got, k, TOL, largest=largest)
    if (name, k, jacobi) not in BODY_COUNT_UNSTABLE:
        within_two_bodies(got, ref)


def test_several_workgroups_and_a_ragged_last_one_in_both_sum_modes(mgcg_env):
    """1287 rows, k = 8: six workgroups in every pass, the last one ragged; 24 columns in the Gram tiles and the combine pass."""
    s = system("poisson13119")
    ref = reference("poisson13119", 8)
    assert ref["status"] == _lib.OK
    got = solve(s, 8)
    check_promises(s, got, 8, TOL)
    within_two_bodies(got, ref)
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    assert_equal_runs(solve(s, 8), ref)


# --------------------------------------------------------------------------- 2. the hierarchy forms, k = 3
@functools.lru_cache(maxsize=None)
def mg_case(name):
    """(system, the yardstick's M^-1, the class's builder)"""
    if name == "box":
        s = system("poisson888")
        H = Hierarchy(*csr_of(s), maps=box_maps(s.grid, 3), omega=class_omega(s.grid))
        return s, H.apply, lambda s, *stop: ConjugateGradientMgGpu(s.Count, _maxnz(s), *stop, s.grid)
    if name == "aggregation":
        s = permuted(system("poisson888"), 7)
        return s, Hierarchy(*csr_of(s)).apply, lambda s, *stop: ConjugateGradientAmgGpu(s.Count, _maxnz(s), *stop)
    s = system("poisson765")
    if name == "ilu":
        return s, IluFactor(*csr_of(s)).apply, lambda s, *stop: ConjugateGradientIluGpu(s.Count, _maxnz(s), *stop)
    return s, GsHierarchy(*csr_of(s), maps=[], nuCoarse=2, omega=1.0).apply, lambda s, *stop: ConjugateGradientSsorGpu(s.Count, _maxnz(s), *stop, omega=1.0)


@functools.lru_cache(maxsize=None)
def mg_reference(name):
    s, minv, _ = mg_case(name)
    return lobpcg_oracle(s, 3, start_block(s.Count, 3), TOL, precond=minv)


def mg_solve(name):
    s, _, make = mg_case(name)
    cg = make(s, 0, 1000, TOL).load(s)
    cg.Initialize()
    out = run(cg, lambda: cg.SolveLobpcg(3, trace=True))
    cg.Dispose()
    return out


MG = ("box", "aggregation", "ilu", "ssor")


@pytest.mark.parametrize("name", MG)
def test_the_hierarchy_form_equals_the_oracle_bit_for_bit(dot_order, name):
    ref = mg_reference(name)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 2
    got = mg_solve(name)
    print(name, "bodies", got["iteration"], ref["iteration"], "theta", got["theta"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("name", MG)
def test_the_hierarchy_form_keeps_the_promises_in_the_default_mode(name):
    got = mg_solve(name)
    check_promises(mg_case(name)[0], got, 3, TOL)
    within_two_bodies(got, mg_reference(name))


def test_a_hierarchy_of_another_size_is_refused(dot_order):
    """The refusal of a hierarchy whose level 0 has not count rows needs a hierarchy, so it is asserted here: nothing is enqueued, the
    object solves with its own hierarchy afterwards."""
    s, small = system("poisson765"), problems.poisson(6, 5, 4)
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, 1000, TOL).load(s)
    other = ConjugateGradientAmgGpu(small.Count, _maxnz(small), 0, 1000, TOL).load(small)
    cg.Initialize()
    other.Initialize()
    with pytest.raises(_lib.MgcgError, match=f"MgcgSolveLobpcgMg: the hierarchy has {small.Count} rows on level 0, the matrix has {s.Count}"):
        cg.SolveLobpcg(3, hierarchy=other)
    assert cg.status == _lib.ERROR and cg.X is None
    cg.SolveLobpcg(3)
    assert cg.status == _lib.OK
    cg.Dispose()
    other.Dispose()


# --------------------------------------------------------------------------- 3. the loop's controls and its breakdowns
def test_a_start_block_with_nan(dot_order):
    s = system("poisson765")
    X0 = start_block(s.Count, 3).copy()
    X0[17, 1] = np.nan
    got = solve(s, 3, X0=X0)
    assert got["status"] == _lib.NONFINITE and got["column_status"] == [_lib.NONFINITE] * 3 and got["iteration"] == -1 and len(got["trace"]) == 0
    assert START_BREAKDOWN in got["message"] and "pivot 1" in got["message"]
    assert np.array_equal(got["X"], X0, equal_nan=True)


def test_count_equal_to_3k(dot_order):
    s = problems.tridiagonal(9)
    ref = lobpcg_oracle(s, 3, start_block(9, 3), TOL)
    got = solve(s, 3)
    print("bodies", got["iteration"], "status", got["status"], ref["fail"])
    assert_equal_runs(got, ref)


def test_a_trace_shorter_than_the_run(dot_order):
    ref = reference("poisson765", 3)
    got = solve(system("poisson765"), 3, trace_capacity=5)
    assert_equal_runs(got, ref, trace_rows=5)


def test_min_iteration_above_the_convergence_point(dot_order):
    first = reference("poisson765", 2)
    min_it = first["iteration"] + 3
    ref = reference("poisson765", 2, min_it=min_it)
    got = solve(system("poisson765"), 2, min_it=min_it)
    assert got["iteration"] >= min_it
    assert_equal_runs(got, ref)


def test_the_cap_is_hit_with_x_still_orthonormal(dot_order):
    ref = reference("poisson765", 4, max_it=7)
    got = solve(system("poisson765"), 4, max_it=7)
    assert got["status"] == _lib.MAXIT_EXCEEDED and got["iteration"] == 7 and _lib.MAXIT_EXCEEDED in got["column_status"]
    assert_equal_runs(got, ref)
    assert np.abs(got["X"].T @ got["X"] - np.eye(4)).max() <= 64 * EPS


def test_two_equal_start_columns(dot_order):
    s = system("poisson765")
    X0 = start_block(s.Count, 3).copy()
    X0[:, 2] = X0[:, 0]
    got = solve(s, 3, X0=X0)
    assert_equal_runs(got, lobpcg_oracle(s, 3, X0, TOL))
    assert got["status"] == _lib.NONFINITE and START_BREAKDOWN in got["message"] and "pivot 2" in got["message"]


def test_exact_eigenvectors_break_w_down(dot_order):
    s = diagonal_system()
    X0 = np.zeros((s.Count, 2))
    X0[3, 0] = X0[7, 1] = 1.0
    got = solve(s, 2, X0=X0, min_it=1)
    assert_equal_runs(got, lobpcg_oracle(s, 2, X0, TOL, min_it=1))
    assert got["status"] == _lib.NONFINITE and W_BREAKDOWN in got["message"] and "pivot 0" in got["message"] and "body 0" in got["message"]
    assert np.array_equal(got["X"], X0) and np.array_equal(got["theta"], [4.0, 8.0])


def test_every_compression_mode_gives_the_same_bits(dot_order):
    s = system("poisson765")
    ref = reference("poisson765", 3)
    for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB):
        assert_equal_runs(solve(s, 3, compression=mode), ref)
