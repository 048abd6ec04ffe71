"""Restarted GMRES(m) on the GPU (SolveGmres, SolveGmresJacobi, gmres.GeneralizedMinimalResidual[Jacobi]Gpu).

The reference for every comparison is ``gmres_oracle`` (tests/test_gmres_host.py): the header's loop in numpy with serial sums.  Under
dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of x and r
must EQUAL it.  In the default mode the summation order differs, and with it the step count, so only the solution's quality is asserted:
numpy's own true residual within 1.001 x the stop level -- the margin of tests/test_gpu_bicgstab.py, which test_gmres_host.py shows to hold
on these inputs with serial sums (estimate and true residual agree to 1e-4 of the level) -- and TrueResidual within 1e-10 relative of it.
Every system but the one streaming-hint case has at most 4097 rows."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib
from conjugategradient_amd.bicgstab import BiConjugateGradientStabGpu
from conjugategradient_amd.gmres import GeneralizedMinimalResidualGpu, GeneralizedMinimalResidualJacobiGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_bicgstab_host import nonsymmetric_tridiagonal, numpy_true_residual, small
from tests.test_gmres_host import CAPS, CONVERGENCE, MS, ORTHS, gmres_oracle, run, singular2, system
from tests.test_sreduce_host import diagonal_of, with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
FORMS = [False, True]
FORM_IDS = ["plain", "jacobi"]
MAX_IT = 20000                                                                     # test_gmres_host.MAX_IT: the shared runs are keyed on it
WHO = {False: "SolveGmres", True: "SolveGmresJacobi"}
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_gmres)
NONFINITE = ("the first residual is zero or not finite, or an Arnoldi step left no next direction and no column (A singular on the Krylov space, "
             "or a value that is not finite)")
# 15 x 15 x 3 c = (5, 5, 5): 675 rows, odd -- the pair tail ; 4097 rows, an uneven diagonal
CORE_SYSTEMS = [("convdiff15x15x3", "randn"), ("random_nonsymmetric4097", "randn")]
# m <= 8 with orth = 1 in the plain form first: one dots and one update launch per pass, no diagonal; then the rest
CORE = sorted(((name, rhs, m, orth, jacobi) for name, rhs in CORE_SYSTEMS for m in MS for orth in ORTHS for jacobi in FORMS),
              key=lambda c: not (c[2] <= 8 and c[3] == 1 and not c[4]))
M, ORTH = 9, 2                                                                     # two launch groups, a restart every ninth step, both passes


def oracle(s, m, orth, jacobi, rule, tol, **kw):
    return gmres_oracle(s, m, orth, 1.0 / diagonal_of(s) if jacobi else None, rule, tol, **kw)


def tolerance(s, rule, rel=1e-8):
    """The relative rule: rel; the absolute rules: rel of the first residual's 2-norm (every system here starts from x = 0: r0 = b)."""
    assert not s.x.any()
    return rel if rule == _lib.RULE_VIENNACL else rel * float(np.linalg.norm(s.b))


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def make(s, m, orth, jacobi, rule, tol, min_it=0, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())
    cls = GeneralizedMinimalResidualJacobiGpu if jacobi else GeneralizedMinimalResidualGpu
    return cls(s.Count, maxnz, min_it, max_it, tol, rule=rule, m=m, orth=orth).load(s)


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


def solve(s, m, orth, jacobi, rule, tol, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None):
    """One solve through the Python class.  prepare(cg): after Initialize()."""
    cg = make(s, m, orth, jacobi, rule, tol, min_it, max_it)
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
@pytest.mark.parametrize("which,rhs,m,orth,jacobi", CORE, ids=[f"{c[0]}-m{c[2]}-orth{c[3]}-{FORM_IDS[c[4]]}" for c in CORE])
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, rhs, m, orth, jacobi):
    s, _ = system(which, rhs)
    ref = run(which, rhs, m, orth, jacobi)                                # RULE_CSHARP to a relative 1e-8, shared with the host tests
    assert ref["status"] == _lib.OK and ref["iteration"] >= 2, ref["iteration"]
    got = solve(s, m, orth, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    print(which, rhs, m, orth, jacobi, "steps", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"],
          "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("rule", RULES)
def test_the_four_rules_from_a_nonzero_guess(dot_order, rule):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, rule)
    start = with_b(s, s.b, "convdiff16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    ref = oracle(start, M, ORTH, False, rule, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] > M
    assert_equal_runs(solve(start, M, ORTH, False, rule, tol), ref)


# --------------------------------------------------------------------------- 2. sizes, minimum, cap, trace
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_tiny_systems_equal_the_oracle(dot_order, n, jacobi):
    """Fewer rows than a workgroup, than a 16-byte pair, than m: the Krylov space is exhausted inside the first cycle (hn = 0 at n = 1)."""
    s = nonsymmetric_tridiagonal(n)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    for m in (M, 32):
        ref = oracle(s, m, ORTH, jacobi, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
        assert ref["status"] == _lib.OK and ref["iteration"] <= n
        assert_equal_runs(solve(s, m, ORTH, jacobi, _lib.RULE_CSHARP, tol), ref)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_min_iteration_beyond_convergence(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = oracle(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tol)
    held = oracle(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 5)
    assert free["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    assert_equal_runs(solve(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 5), held)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("cap", [12, 8, 3])
def test_iteration_cap_equals_the_oracle(dot_order, cap, jacobi):
    """The close in mid-cycle (cap 12: four steps into the second cycle), at the cycle's end (8) and inside the first (3)."""
    s, _ = system("convdiff16", "randn")
    ref = oracle(s, M, ORTH, jacobi, _lib.RULE_CSHARP, 0.0, max_it=cap)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == cap + 1
    got = solve(s, M, ORTH, jacobi, _lib.RULE_CSHARP, 0.0, max_it=cap)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message(WHO[jacobi], got, cap)]


def test_a_trace_shorter_than_the_run(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    ref = dict(run("convdiff15x15x3", "randn", M, ORTH, False))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, M, ORTH, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP), trace_capacity=5), ref)


def test_the_streaming_hint_form(dot_order):
    """3 000 001 rows: above the threshold of the streaming hint, odd.  m = 9 and a cap of 12: a restart and two launch groups."""
    s = nonsymmetric_tridiagonal(3000001)
    ref = oracle(s, M, ORTH, False, _lib.RULE_CSHARP, 0.0, max_it=12)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 13
    assert_equal_runs(solve(s, M, ORTH, False, _lib.RULE_CSHARP, 0.0, max_it=12), ref)


# --------------------------------------------------------------------------- 3. matrix forms, work space, corner cases
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tol, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], run("convdiff16", "randn", M, ORTH, jacobi))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, jacobi):
    """NaN in the whole work vector and in p, Ap and r."""
    s, _ = system("convdiff15x15x3", "randn")
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        size = (M + 1 + cg._slices_more) * (s.Count + (s.Count & 1))      # all of it
        assert cg._work_size == size
        cg.vectorWork.CopyFrom(np.full(size, np.nan), size)
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR):
            v.CopyFrom(nan, s.Count)
        dvec(nan).Dispose()

    assert_equal_runs(solve(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP), prepare=prepare), run("convdiff15x15x3", "randn", M, ORTH, jacobi))


def test_the_singular_branch_gives_nonfinite_and_the_callers_x_back(dot_order):
    """d = 0 in step 0.  The zero diagonal is no diagonal for the Jacobi set-up to take: the plain form only."""
    s = singular2()
    ref = oracle(s, M, ORTH, False, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], s.x)
    got = solve(s, M, ORTH, False, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message(WHO[False], got, NONFINITE)]


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_the_exhausted_branch_ends_ok_whatever_the_minimum_says(dot_order, jacobi):
    """[[1, 1], [0, 1]], b = (0, 1): hn = 0 exactly in the second step (tests/test_gmres_host.py derives it).  Diagonal (1, 1)."""
    s = small([[1.0, 1.0], [0.0, 1.0]], [0.0, 1.0], "exhausted2", x=[0.0, 0.0])
    ref = oracle(s, M, ORTH, jacobi, _lib.RULE_CSHARP, 0.0, min_it=5)
    assert ref["status"] == _lib.OK and ref["iteration"] == 2 and ref["residual"] == 0.0
    assert_equal_runs(solve(s, M, ORTH, jacobi, _lib.RULE_CSHARP, 0.0, min_it=5), ref)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_zero_right_hand_side_gives_nonfinite(dot_order, jacobi):
    s = nonsymmetric_tridiagonal(50)
    zero = with_b(s, np.zeros(50), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = oracle(zero, M, ORTH, jacobi, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        assert_equal_runs(solve(zero, M, ORTH, jacobi, rule, 1e-12), ref)


# --------------------------------------------------------------------------- 4. the capability
def _bicgstab_outcome(s, tol):
    """SolveBicgstab on the same system: (object, status)."""
    maxnz = int(np.diff(s.RowOffsets).max())
    old = BiConjugateGradientStabGpu(s.Count, maxnz, 0, 3000, tol, rule=_lib.RULE_CSHARP).load(s)
    old.Initialize()
    try:
        old.Solve()
    except (_lib.MgcgError, ApplicationException):
        pass
    return old


@pytest.mark.parametrize("m", [20, 5])
def test_gmres_converges_where_bicgstab_breaks_down(dot_order, m):
    s, _ = system("convdiff32x32_20", "ones")
    tol = tolerance(s, _lib.RULE_CSHARP)
    old = _bicgstab_outcome(s, tol)
    print("SolveBicgstab: status", old.status, "at body", old.Iteration, "TrueResidual", old.TrueResidual / tol, "x the level")
    assert old.status == _lib.NONFINITE
    old.Dispose()
    got = solve(s, m, ORTH, False, _lib.RULE_CSHARP, tol, max_it=CAPS["convdiff32x32_20"])
    true = numpy_true_residual(s, got["x"])
    print(f"SolveGmres({m}):", got["iteration"], "steps, TrueResidual", got["true_residual"] / tol, "numpy", true / tol, "x the level")
    assert got["status"] == _lib.OK and got["true_residual"] <= 1.001 * tol and true <= 1.001 * tol


def test_gmres_does_not_drift_where_bicgstab_does(dot_order):
    s, _ = system("tridiagonal300_19", "ones")
    tol = tolerance(s, _lib.RULE_CSHARP)
    old = _bicgstab_outcome(s, tol)
    print("SolveBicgstab: status", old.status, "Residual", old.Residual, "TrueResidual", old.TrueResidual)
    assert not (old.TrueResidual <= 1e6 * max(old.Residual, tol))                 # far above its recurrence's figure, or not a number
    old.Dispose()
    got = solve(s, 20, ORTH, False, _lib.RULE_CSHARP, tol, max_it=CAPS["tridiagonal300_19"])
    true = numpy_true_residual(s, got["x"])
    print("SolveGmres(20):", got["iteration"], "steps, TrueResidual", got["true_residual"] / tol, "numpy", true / tol, "x the level")
    assert got["status"] == _lib.OK and got["true_residual"] <= 1.001 * tol and true <= 1.001 * tol


# --------------------------------------------------------------------------- 5. default mode
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("m,orth", [(20, 2), (9, 1)])
@pytest.mark.parametrize("rhs", ["ones", "randn"])
@pytest.mark.parametrize("which", CONVERGENCE)
def test_default_dot_order_solves_every_system(which, rhs, m, orth, jacobi):
    s, _ = system(which, rhs)
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, m, orth, jacobi, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, got["x"])
    print(which, rhs, m, orth, jacobi, "steps", got["iteration"], "estimate", got["residual"], "TrueResidual", got["true_residual"],
          "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == _lib.OK
    assert true <= 1.001 * tol
    assert abs(got["true_residual"] - true) <= 1e-10 * true


# --------------------------------------------------------------------------- 6. the object and the C call
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_second_solve_on_the_same_object_gives_the_same_result(dot_order, jacobi):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, M, ORTH, jacobi, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    cg.Initialize()
    first = finish(cg)
    cg.x[:] = 0.0
    cg.Initialize()
    second = finish(cg)
    cg.Dispose()
    assert_equal_runs(first, run("convdiff15x15x3", "randn", M, ORTH, jacobi))
    assert_equal_runs(second, first)


def test_the_class_method_gives_the_c_calls_result(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = run("convdiff15x15x3", "randn", 17, 1, False)
    cg = make(s, 17, 1, False, _lib.RULE_CSHARP, tol)
    cg.Initialize()
    by_class = finish(cg)
    # the same call by hand, on the object's own vectors
    cg.vectorX.CopyFrom(np.zeros(s.Count), s.Count)
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    st = _lib.lib().SolveGmres(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                               cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, cg.vectorWork.Ptr,
                               17, 1, s.nnz, s.Count, tol, 0, MAX_IT, _lib.RULE_CSHARP, C.byref(it), C.byref(res), C.byref(true), None, 0)
    cg.Read()
    assert (st, it.value, res.value, true.value) == (ref["status"], ref["iteration"], ref["residual"], ref["true_residual"])
    assert np.array_equal(cg.x, ref["x"]) and np.array_equal(cg.ReadResidual(), ref["r"])
    assert_equal_runs(by_class, ref)
    cg.Dispose()


def test_a_refused_m_leaves_the_object_able_to_solve(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, 33, ORTH, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="m = 33, must be 1 .. 32"):
        cg.Solve()
    assert cg.status == _lib.ERROR
    cg.m = M
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", M, ORTH, False))
    cg.Dispose()


def test_a_raised_m_gets_a_larger_work_vector(dot_order):
    s, _ = system("convdiff15x15x3", "randn")
    cg = make(s, 2, ORTH, False, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
    stride = s.Count + (s.Count & 1)
    assert cg._work_size == 3 * stride
    cg.Initialize()
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", 2, ORTH, False))
    cg.m = 17
    cg.x[:] = 0.0
    cg.Initialize()
    assert_equal_runs(finish(cg), run("convdiff15x15x3", "randn", 17, ORTH, False))
    assert cg._work_size == 18 * stride
    cg.Dispose()
