"""BiCGStab on the GPU (SolveBicgstab*, SolveBicgstabJacobi*, bicgstab.BiConjugateGradientStab[Jacobi]Gpu,
ConjugateGradientRankGpu.SolveBicgstab[Jacobi]).

The reference for every comparison is ``bicgstab_oracle`` (tests/test_bicgstab_host.py): the header's loop in numpy with serial sums.
Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of
x and r must EQUAL it.  In the default mode the summation order differs, and with it the iteration count (the yardstick's own count moves
365 / 368 / 367 on the tridiagonal matrix between serial, pairwise and exactly rounded sums), so only the solution's quality is asserted:
the true residual within 1.001 x the stop level, which test_bicgstab_host.py shows to be safe on these inputs."""
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.bicgstab import BiConjugateGradientStabGpu, BiConjugateGradientStabJacobiGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_bicgstab_host import (CASES, bicgstab_oracle, nonsymmetric_tridiagonal, numpy_true_residual, rho_zero2, sigma_zero2,
                                      system)
from tests.test_gpu_jacobi import run_ranks
from tests.test_sreduce_host import diagonal_of, with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
FORMS = [False, True]
FORM_IDS = ["plain", "jacobi"]
MAX_IT = 3000
_oracles = {}
WHO = {False: "SolveBicgstab", True: "SolveBicgstabJacobi"}
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_bicgstab)
NONFINITE = "the first residual is zero or not finite, or the recurrence broke down (rhat.v, omega or rhat.r zero, or a value that is not finite)"


def reference(name, rhs, jacobi, rule, tol, parts=None, **kw):
    """The oracle's run, computed once per case and shared (nothing changes it)."""
    key = (name, rhs, jacobi, rule, tol, None if parts is None else tuple(parts), tuple(sorted(kw.items())))
    if key not in _oracles:
        s, dinv = system(name, rhs)
        _oracles[key] = bicgstab_oracle(s, dinv if jacobi else None, rule, tol, parts=parts, **{"max_it": MAX_IT, **kw})
    return _oracles[key]


def oracle(s, jacobi, rule, tol, **kw):
    return bicgstab_oracle(s, 1.0 / diagonal_of(s) if jacobi else None, rule, tol, **kw)


def tolerance(s, rule, rel=1e-8):
    """The relative rule: rel; the absolute rules: rel of the first residual's 2-norm (every system here starts from x = 0: r0 = b)."""
    assert not s.x.any()
    return rel if rule == _lib.RULE_VIENNACL else rel * float(np.linalg.norm(s.b))


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def solve(s, jacobi, rule, tol, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None):
    """One solve through the Python class; an iteration cap that was hit or a breakdown is a result here, not an exception.
    prepare(cg): after Initialize()."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cls = BiConjugateGradientStabJacobiGpu if jacobi else BiConjugateGradientStabGpu
    cg = cls(s.Count, maxnz, min_it, max_it, tol, rule=rule).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    if prepare is not None:
        prepare(cg)
    with library_messages() as said:
        try:
            cg.Solve(trace=True, traceCapacity=trace_capacity)
        except ApplicationException:
            assert cg.status == _lib.MAXIT_EXCEEDED
        except _lib.MgcgError:
            assert cg.status == _lib.NONFINITE
    cg.Read()
    out = dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual,
               status=cg.status, trace=cg.trace, messages=list(said))
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
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which,rhs", CASES)
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, rhs, jacobi, rule):
    s, _ = system(which, rhs)
    tol = tolerance(s, rule)
    ref = reference(which, rhs, jacobi, rule, tol)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, jacobi, rule, tol)
    print(which, rhs, jacobi, rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"],
          "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 2. sizes, start, minimum, cap, trace
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", [1, 2, 7, 300, 771])
def test_small_and_odd_sizes_equal_the_oracle(dot_order, n, jacobi):
    """Less than a workgroup, no multiple of 256 or of the 16-byte access, more than one workgroup."""
    s = nonsymmetric_tridiagonal(n)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = oracle(s, jacobi, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK
    assert_equal_runs(solve(s, jacobi, _lib.RULE_CSHARP, tol), ref)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_nonzero_initial_guess(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    start = with_b(s, s.b, "convdiff16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = oracle(start, jacobi, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, jacobi, _lib.RULE_CSHARP, tol), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, jacobi, _lib.RULE_SIMPLE, tol), reference("convdiff16", "randn", jacobi, _lib.RULE_SIMPLE, tol))


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_min_iteration_beyond_convergence(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = oracle(s, jacobi, _lib.RULE_CSHARP, tol)
    held = oracle(s, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, jacobi, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6), held)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_iteration_cap_equals_the_oracle(dot_order, jacobi):
    ref = reference("convdiff16", "randn", jacobi, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(system("convdiff16", "randn")[0], jacobi, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message(WHO[jacobi], got, 3)]          # "SolveBicgstab: did not converge: iteration 4 exceeded maxIteration 3 (residual ...)"


def test_the_iteration_cap_raises_application_exception(dot_order):
    s, _ = system("convdiff16", "randn")
    cg = BiConjugateGradientStabGpu(s.Count, 7, 0, 3, 0.0, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    with pytest.raises(ApplicationException):
        cg.Solve()
    cg.Read()
    assert cg.status == _lib.MAXIT_EXCEEDED and np.array_equal(cg.x, reference("convdiff16", "randn", False, _lib.RULE_CSHARP, 0.0, max_it=3)["x"])
    cg.Dispose()


def test_a_trace_shorter_than_the_run(dot_order):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = dict(reference("convdiff16", "randn", False, _lib.RULE_CSHARP, tol))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, False, _lib.RULE_CSHARP, tol, trace_capacity=5), ref)


# --------------------------------------------------------------------------- 3. default mode
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which,rhs", CASES)
def test_default_dot_order_solves_every_case(which, rhs, jacobi):
    s, _ = system(which, rhs)
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, jacobi, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, got["x"])
    print(which, rhs, jacobi, "iterations", got["iteration"], "recurrence", got["residual"], "TrueResidual", got["true_residual"],
          "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == _lib.OK
    assert true <= 1.001 * tol
    assert abs(got["true_residual"] - true) <= 1e-10 * true


def test_a_symmetric_system_agrees_with_plain_cg():
    s, _ = system("poisson16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, False, _lib.RULE_CSHARP, tol)
    cg = ConjugateGradientSingleGpu(s.Count, 7, 0, MAX_IT, tol, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    cg.Solve()
    cg.Read()
    distance = float(np.linalg.norm(got["x"] - cg.x) / np.linalg.norm(cg.x))
    cg.Dispose()
    print("poisson16: BiCGStab", got["iteration"], "bodies, distance to CG's x", distance)
    assert got["status"] == _lib.OK and distance <= 1e-6


# --------------------------------------------------------------------------- 4. matrix forms, work space, corner cases
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, jacobi):
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, jacobi, _lib.RULE_CSHARP, tol, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], reference("convdiff16", "randn", jacobi, _lib.RULE_CSHARP, tol))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, jacobi):
    """NaN in all seven work vectors."""
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR, cg.vectorV, cg.vectorS, cg.vectorT, cg.vectorRhat):
            v.CopyFrom(nan, s.Count)
        dvec(nan).Dispose()

    assert_equal_runs(solve(s, jacobi, _lib.RULE_CSHARP, tol, prepare=prepare), reference("convdiff16", "randn", jacobi, _lib.RULE_CSHARP, tol))


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_sigma_zero_gives_nonfinite_and_the_callers_x_back(dot_order, jacobi):
    s = sigma_zero2()                                       # diagonal (1, 1): the Jacobi form takes the same steps
    ref = oracle(s, jacobi, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], s.x)
    got = solve(s, jacobi, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message(WHO[jacobi], got, NONFINITE)]
    started = with_b(s, s.b, "sigma_zero2-x0")
    started.x[:] = [0.0, 1.0]
    ok = oracle(started, jacobi, _lib.RULE_CSHARP, 1e-12)
    assert ok["status"] == _lib.OK
    assert_equal_runs(solve(started, jacobi, _lib.RULE_CSHARP, 1e-12), ok)


def test_rhon_zero_gives_nonfinite_with_this_bodys_iterate(dot_order):
    s = rho_zero2()
    ref = oracle(s, False, _lib.RULE_CSHARP, 0.0)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], [0.5, 0.0])
    assert_equal_runs(solve(s, False, _lib.RULE_CSHARP, 0.0), ref)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_zero_right_hand_side_gives_nonfinite(dot_order, jacobi):
    s = nonsymmetric_tridiagonal(50)
    zero = with_b(s, np.zeros(50), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = oracle(zero, jacobi, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        assert_equal_runs(solve(zero, jacobi, rule, 1e-12), ref)


# --------------------------------------------------------------------------- 5. the streaming-hint form of the passes
STREAMING_ROWS = 3_000_001      # the smallest row count at which the passes take their streaming-hint form (n > 3 000 000); odd: the tail element runs
_streaming = {}


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_streaming_hint_form_equals_the_oracle(dot_order, jacobi):
    """Three forced bodies, tolerance 0, so that both sides stop at the iteration cap.  The one test beyond 5000 rows: the form exists
    only beyond 3 000 000."""
    if "s" not in _streaming:
        _streaming["s"] = nonsymmetric_tridiagonal(STREAMING_ROWS)
    s = _streaming["s"]
    ref = oracle(s, jacobi, _lib.RULE_CSHARP, 0.0, max_it=2)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 3
    assert_equal_runs(solve(s, jacobi, _lib.RULE_CSHARP, 0.0, max_it=2), ref)


# --------------------------------------------------------------------------- 6. ranks
def _rank_solve(s, world, jacobi, rule, tol, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, max_it, tol, rank=rank, world=world, comm=comm, rule=rule, device=rank).load(s)
        cg.Initialize()
        if jacobi:
            cg.SetupJacobi()
            cg.SolveBicgstabJacobi(trace=True)
        else:
            cg.SolveBicgstab(trace=True)
        cg.Read()
        p = cg.part
        r = np.zeros(max(p.count, 1))
        if p.count:
            cg.vectorR.CopyTo(r, p.count, 0)
        out = dict(offset=p.offset, count=p.count, x=cg.x[p.offset: p.offset + p.count].copy(), r=r[: p.count], iteration=cg.Iteration,
                   residual=cg.Residual, true_residual=cg.TrueResidual, status=cg.status, trace=cg.trace)
        cg.Dispose()
        return out

    return run_ranks(world, make_rank)


def _assert_ranks_equal(res, ref, parts):
    x, r = np.zeros(parts[-1]), np.zeros(parts[-1])
    for k in res:
        x[k["offset"]: k["offset"] + k["count"]] = k["x"]
        r[k["offset"]: k["offset"] + k["count"]] = k["r"]
        assert k["status"] == ref["status"] and k["iteration"] == ref["iteration"] and k["residual"] == ref["residual"]
        assert k["true_residual"] == ref["true_residual"]
        assert np.array_equal(k["trace"], ref["trace"])
    assert [k["offset"] for k in res] == parts[:-1]
    assert np.array_equal(x, ref["x"])
    assert np.array_equal(r, ref["r"])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which", ["convdiff16", "random_nonsymmetric5000"])
def test_ranks_equal_the_oracle_with_its_sums_cut_at_their_rows(mgcg_env, dot_order, which, jacobi, world):
    """random_nonsymmetric5000: the halo is an index list, and what a rank needs from its neighbours is not what they need from it."""
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s, _ = system(which, "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    parts = problems.partition_offsets(s.Count, world)
    ref = reference(which, "randn", jacobi, _lib.RULE_CSHARP, tol, parts=parts)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    _assert_ranks_equal(_rank_solve(s, world, jacobi, _lib.RULE_CSHARP, tol), ref, parts)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_a_rank_without_rows_takes_part(mgcg_env, dot_order, jacobi):
    world = 4
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = nonsymmetric_tridiagonal(3)                     # 3 rows over 4 ranks: offsets [0, 0, 0, 0, 3]
    parts = problems.partition_offsets(s.Count, world)
    assert parts == [0, 0, 0, 0, 3]
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = oracle(s, jacobi, _lib.RULE_CSHARP, tol, max_it=50, parts=parts)
    assert ref["status"] == _lib.OK
    res = _rank_solve(s, world, jacobi, _lib.RULE_CSHARP, tol, max_it=50)
    assert [k["count"] for k in res] == [0, 0, 0, 3]
    _assert_ranks_equal(res, ref, parts)


@pytest.mark.parametrize("jacobi", FORMS, ids=FORM_IDS)
def test_the_forced_several_ranks_path_on_one_rank_equals_the_one_rank_loop(mgcg_env, dot_order, jacobi):
    """MGCG_FORCE_MULTIRANK: a one-rank RCCL communicator takes the fold / all-reduce / GIVEN-pass path with a real ncclAllReduce on the
    stream; the sums are the one-rank loop's, so are the bits."""
    import ctypes as C

    L = _lib.lib()
    L.SetDevice(0)
    buf = (C.c_char * 128)()
    assert L.MgcgCommGetUniqueId(buf) == 0, _lib.last_error()
    comm = L.MgcgCommInitRank(buf, 1, 0)
    assert comm, _lib.last_error()
    mgcg_env.setenv("MGCG_FORCE_MULTIRANK", "1")
    s, _ = system("convdiff16", "randn")
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, MAX_IT, tol, rank=0, world=1, comm=comm, rule=_lib.RULE_CSHARP, device=0).load(s)
    cg.Initialize()
    if jacobi:
        cg.SetupJacobi()
    cg.SolveBicgstab(trace=True, jacobi=jacobi)
    cg.Read()
    r = np.zeros(s.Count)
    cg.vectorR.CopyTo(r, s.Count, 0)
    got = dict(x=cg.x.copy(), r=r, iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual, status=cg.status, trace=cg.trace)
    cg.Dispose()
    assert_equal_runs(got, reference("convdiff16", "randn", jacobi, _lib.RULE_CSHARP, tol))
    L.MgcgCommDestroy(comm)
