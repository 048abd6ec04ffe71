"""BiCGStab(l) on the GPU (SolveBicgstabL, SolveBicgstabLJacobi, bicgstab.BiConjugateGradientStabL[Jacobi]Gpu).

The reference for every comparison is ``bicgstabl_oracle`` (tests/test_bicgstabl_host.py): the header's loop in numpy with serial sums.
Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of
x and r must EQUAL it.  In the default mode the summation order differs, and with it the body count, so only the solution's quality is
asserted: numpy's own true residual within 1.001 x the stop level -- the margin of tests/test_gpu_bicgstab.py, which
test_bicgstabl_host.py shows to hold on these inputs with serial sums -- and TrueResidual within 1e-10 relative of it.  Every system has
at most 4097 rows."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib
from conjugategradient_amd.bicgstab import (BiConjugateGradientStabGpu, BiConjugateGradientStabLGpu, BiConjugateGradientStabLJacobiGpu)
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_bicgstab_host import nonsymmetric_tridiagonal, numpy_true_residual, small
from tests.test_bicgstabl_host import ELLS, MIN_ELL, bicgstabl_oracle, run, system, two_cycle
from tests.test_sreduce_host import diagonal_of, with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
FORMS = [False, True]
FORM_IDS = ["plain", "jacobi"]
MAX_IT = 3000
WHO = {False: "SolveBicgstabL", True: "SolveBicgstabLJacobi"}
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_bicgstabl)
NONFINITE = "the first residual is zero or not finite, or the recurrence broke down (rt.u_{j+1}, omega or rt.r_0 zero, or a value that is not finite)"
# 16^3 c = (.5, .25, 0) ; 32^2 c = (20, 20, 0), where BiCGStab breaks down ; 15 x 15 x 3 c = (5, 5, 5): 675 rows, odd -- the pair tail ;
# 4097 rows, an uneven diagonal
SYSTEMS = [("convdiff16", "randn"), ("convdiff32x32_20", "ones"), ("convdiff15x15x3", "randn"), ("random_nonsymmetric4097", "randn")]
CASES = [(name, rhs, ell) for name, rhs in SYSTEMS for ell in ELLS if ell >= MIN_ELL.get(name, 1)]


def oracle(s, ell, jacobi, rule, tol, **kw):
    return bicgstabl_oracle(s, ell, 1.0 / diagonal_of(s) if jacobi else None, rule, tol, **kw)


def tolerance(s, rule, rel=1e-8):
    """The relative rule: rel; the absolute rules: rel of the first residual's 2-norm (every system here starts from x = 0: r0 = b)."""
    assert not s.x.any()
    return rel if rule == _lib.RULE_VIENNACL else rel * float(np.linalg.norm(s.b))


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def make(s, ell, jacobi, rule, tol, min_it=0, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())
    cls = BiConjugateGradientStabLJacobiGpu if jacobi else BiConjugateGradientStabLGpu
    return cls(s.Count, maxnz, min_it, max_it, tol, rule=rule, ell=ell).load(s)


def finish(cg, trace_capacity=None):
    """Solve() and read everything back; an iteration cap that was hit or a breakdown is a result here, not an exception."""
    with library_messages() as said:
        try:
            cg.Solve(trace=True, traceCapacity=trace_capacity)
        except ApplicationException:
            assert cg.status == _lib.MAXIT_EXCEEDED
        except _lib.MgcgError:
            assert cg.status == _lib.NONFINITE
    cg.Read()
    return dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual,
                status=cg.status, trace=cg.trace, messages=list(said))


def solve(s, ell, jacobi, rule, tol, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None):
    """One solve through the Python class.  prepare(cg): after Initialize()."""
    cg = make(s, ell, jacobi, rule, tol, min_it, max_it)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    if prepare is not None:
        prepare(cg)
    out = finish(cg, trace_capacity)
    cg.Dispose()
    return out


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert same(got["residual"], ref["residual"]), (got["residual"], ref["residual"])
    assert same(got["true_residual"], ref["true_residual"]), (got["true_residual"], ref["true_residual"])
    assert np.array_equal(got["trace"], ref["trace"], equal_nan=True)
    assert np.array_equal(got["x"], ref["x"], equal_nan=True)
    assert np.array_equal(got["r"], ref["r"], equal_nan=True)


# --------------------------------------------------------------------------- 1. bit equality with the oracle
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which,rhs,ell", CASES)
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, rhs, ell, jacobi):
    s, _ = system(which, rhs)
    ref = run(which, rhs, ell, jacobi)                                    # RULE_CSHARP to a relative 1e-8, shared with the host tests
    assert ref["status"] == _lib.OK and ref["iteration"] >= 2, ref["iteration"]
    got = solve(s, ell, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    print(which, rhs, ell, jacobi, "bodies", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"],
          "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("ell", [2, 4])
@pytest.mark.parametrize("rule", RULES)
def test_the_four_rules(dot_order, rule, ell):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, rule)
    ref = oracle(s, ell, False, rule, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(s, ell, False, rule, tol), ref)


# --------------------------------------------------------------------------- 2. sizes, start, minimum, cap, trace
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_systems_equal_the_oracle(dot_order, n, ell, jacobi):
    """Fewer rows than a workgroup, than a 16-byte pair, than l: the Krylov space is exhausted inside the first body."""
    s = nonsymmetric_tridiagonal(n)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = oracle(s, ell, jacobi, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] in (_lib.OK, _lib.NONFINITE)
    assert_equal_runs(solve(s, ell, jacobi, _lib.RULE_CSHARP, tol), ref)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [2, 3])
def test_a_nonzero_initial_guess(dot_order, ell, jacobi):
    s, _ = system("convdiff16", "randn")
    start = with_b(s, s.b, "convdiff16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = oracle(start, ell, jacobi, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, ell, jacobi, _lib.RULE_CSHARP, tol), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, ell, jacobi, _lib.RULE_SIMPLE, tol), oracle(s, ell, jacobi, _lib.RULE_SIMPLE, tol, max_it=MAX_IT))


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [1, 4])
def test_min_iteration_beyond_convergence(dot_order, ell, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = oracle(s, ell, jacobi, _lib.RULE_CSHARP, tol)
    held = oracle(s, ell, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 3)
    assert free["status"] == _lib.OK and held["iteration"] >= free["iteration"] + 3
    assert_equal_runs(solve(s, ell, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 3), held)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [2, 4])
def test_iteration_cap_equals_the_oracle(dot_order, ell, jacobi):
    s, _ = system("convdiff16", "randn")
    ref = oracle(s, ell, jacobi, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(s, ell, jacobi, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message(WHO[jacobi], got, 3)]


def test_a_trace_shorter_than_the_run(dot_order):
    s, _ = system("convdiff16", "randn")
    ref = dict(run("convdiff16", "randn", 2, False))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, 2, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP), trace_capacity=5), ref)


# --------------------------------------------------------------------------- 3. matrix forms, work space, corner cases
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, 2, jacobi, _lib.RULE_CSHARP, tol, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], run("convdiff16", "randn", 2, jacobi))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [2, 4])
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, ell, jacobi):
    """NaN in the whole work vector and in p, Ap and r."""
    s, _ = system("convdiff16", "randn")
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        size = (2 * ell + cg._slices_more) * (s.Count + (s.Count & 1))    # all of it
        assert cg._work_size == size
        cg.vectorWork.CopyFrom(np.full(size, np.nan), size)
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR):
            v.CopyFrom(nan, s.Count)
        dvec(nan).Dispose()

    assert_equal_runs(solve(s, ell, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP), prepare=prepare), run("convdiff16", "randn", ell, jacobi))


@pytest.mark.parametrize("ell", ELLS)
def test_sigma_zero_at_step_0_gives_nonfinite_and_the_callers_x_back(dot_order, ell):
    """The rotation by 90 degrees has no diagonal for the Jacobi set-up to take: the plain form only."""
    s = two_cycle()
    ref = oracle(s, ell, False, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], s.x)
    got = solve(s, ell, False, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message(WHO[False], got, NONFINITE)]


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [2, 3, 4])
def test_sigma_zero_at_step_1_leaves_what_step_0_made(dot_order, ell, jacobi):
    """tests/test_bicgstabl_host.py derives it: x = (1, 0, 0) and r_0 = (0, 0, 1) after step 0, sigma = 0 in step 1.  Diagonal (1, 1, 1)."""
    s = small([[1.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 1.0]], [1.0, 0.0, 0.0], "sigma_zero_at_step_1", x=[0.0, 0.0, 0.0])
    ref = oracle(s, ell, jacobi, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], [1.0, 0.0, 0.0])
    got = solve(s, ell, jacobi, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message(WHO[jacobi], got, NONFINITE)]


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ell", [1, 3])
def test_a_zero_right_hand_side_gives_nonfinite(dot_order, ell, jacobi):
    s = nonsymmetric_tridiagonal(50)
    zero = with_b(s, np.zeros(50), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = oracle(zero, ell, jacobi, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        assert_equal_runs(solve(zero, ell, jacobi, rule, 1e-12), ref)


# --------------------------------------------------------------------------- 4. the capability
def test_bicgstab_breaks_down_where_ell_2_converges(dot_order):
    s, _ = system("convdiff32x32_20", "ones")
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    old = BiConjugateGradientStabGpu(s.Count, maxnz, 0, MAX_IT, tol, rule=_lib.RULE_CSHARP).load(s)
    old.Initialize()
    with pytest.raises(_lib.MgcgError):
        old.Solve()
    print("SolveBicgstab: status", old.status, "at body", old.Iteration, "TrueResidual", old.TrueResidual / tol, "x the level")
    assert old.status == _lib.NONFINITE
    # the same matrix, right-hand side and start, as the first object holds them
    new = BiConjugateGradientStabLGpu(s.Count, maxnz, 0, MAX_IT, tol, rule=_lib.RULE_CSHARP, ell=2)
    new.A, new.x, new.b = old.A, old.x, old.b
    new.x[:] = 0.0
    new.Initialize()
    new.Solve()
    new.Read()
    true = numpy_true_residual(s, new.x)
    print("SolveBicgstabL(2):", new.Iteration, "bodies, TrueResidual", new.TrueResidual / tol, "numpy", true / tol, "x the level")
    assert new.status == _lib.OK and new.TrueResidual <= 1.001 * tol and true <= 1.001 * tol
    old.Dispose()
    new.Dispose()


# --------------------------------------------------------------------------- 5. default mode
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which,rhs,ell", CASES)
def test_default_dot_order_solves_every_case(which, rhs, ell, jacobi):
    s, _ = system(which, rhs)
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, ell, jacobi, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, got["x"])
    print(which, rhs, ell, jacobi, "bodies", got["iteration"], "recurrence", got["residual"], "TrueResidual", got["true_residual"],
          "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == _lib.OK
    assert true <= 1.001 * tol
    assert abs(got["true_residual"] - true) <= 1e-10 * true


@pytest.mark.parametrize("rule", RULES)
def test_default_dot_order_under_every_rule_from_a_nonzero_guess(rule):
    """l = 2 on 15 x 15 x 3, c = (5, 5, 5): each rule's own test, a start that MGCG_RULE_SIMPLE replaces by 0, a minimum of two bodies."""
    s, _ = system("convdiff15x15x3", "randn")
    tol = tolerance(s, rule)
    start = with_b(s, s.b, "convdiff15x15x3-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    got = solve(start, 2, False, rule, tol, min_it=2)
    # the relative rule measures against the first residual b - A x0, the others against the absolute tolerance
    level = 1e-8 * float(np.linalg.norm(s.b - _first_product(start))) if rule == _lib.RULE_VIENNACL else tol
    true = numpy_true_residual(s, got["x"])
    print("rule", rule, "bodies", got["iteration"], "TrueResidual", got["true_residual"], "numpy", true, "=", true / level, "x the stop level")
    assert got["status"] == _lib.OK and got["iteration"] >= 3
    assert true <= 1.001 * level
    assert abs(got["true_residual"] - true) <= 1e-10 * true


def _first_product(s):
    """A x of the system's own start."""
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * s.x[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


# --------------------------------------------------------------------------- 6. the object and the C call
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_second_solve_on_the_same_object_gives_the_same_result(dot_order, jacobi):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, 2, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    cg.Initialize()
    first = finish(cg)
    cg.x[:] = 0.0
    cg.Initialize()
    second = finish(cg)
    cg.Dispose()
    assert_equal_runs(first, run("convdiff15x15x3", "randn", 2, jacobi))
    assert_equal_runs(second, first)


def test_the_class_method_gives_the_c_calls_result(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = run("convdiff15x15x3", "randn", 3, False)
    cg = make(s, 3, False, _lib.RULE_CSHARP, tol)
    cg.Initialize()
    by_class = finish(cg)
    # the same call by hand, on the object's own vectors
    cg.vectorX.CopyFrom(np.zeros(s.Count), s.Count)
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    st = _lib.lib().SolveBicgstabL(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                                   cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, cg.vectorWork.Ptr,
                                   3, s.nnz, s.Count, tol, 0, MAX_IT, _lib.RULE_CSHARP, C.byref(it), C.byref(res), C.byref(true), None, 0)
    cg.Read()
    assert (st, it.value, res.value, true.value) == (ref["status"], ref["iteration"], ref["residual"], ref["true_residual"])
    assert np.array_equal(cg.x, ref["x"]) and np.array_equal(cg.ReadResidual(), ref["r"])
    assert_equal_runs(by_class, ref)
    cg.Dispose()


def test_a_refused_ell_leaves_the_object_able_to_solve(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, 5, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="ell = 5, must be 1 .. 4"):
        cg.Solve()
    assert cg.status == _lib.ERROR
    cg.ell = 2
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", 2, False))
    cg.Dispose()


def test_a_raised_ell_gets_a_larger_work_vector(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, 1, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    stride = s.Count + (s.Count & 1)
    assert cg._work_size == 2 * stride
    cg.Initialize()
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", 1, False))
    cg.ell = 4
    cg.x[:] = 0.0
    cg.Initialize()
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", 4, False))
    assert cg._work_size == 8 * stride
    cg.Dispose()
