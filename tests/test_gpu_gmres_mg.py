"""V-cycle-preconditioned flexible GMRES(m) on the GPU (SolveGmresMg, ConjugateGradientMgGpu.SolveGmres, inherited by
ConjugateGradientAmgGpu and ConjugateGradientSsorGpu).

The reference for every comparison is ``fgmres_oracle`` with ``Hierarchy.apply`` as M^-1 (tests/test_gmres_mg_host.py,
tests/test_amg_host.py): the header's loop and the cycle in numpy with serial sums.  Under dot_order = 1 the HIP loop is a fixed sequence of
IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of x and r must EQUAL it.  In the default mode the summation
order differs, and with it the step count, so only the solution's quality is asserted: numpy's own true residual within 1.001 x the stop
level, which test_gmres_mg_host.py shows to be safe on these inputs (estimate and true residual agree to 1e-4 of the level with serial
sums), and TrueResidual within 1e-10 relative of it.  That the set-up paths give the yardstick's hierarchies on nonsymmetric matrices is
tests/test_gpu_bicgstab_mg.py's first section.

The streaming-hint form (3 000 001 rows, a one-level hierarchy, m = 2, 3 steps) is left out: its numpy yardstick alone takes 5.8 s, and the
system and its hierarchy 0.9 s more -- not "a few seconds".  The passes that take the hint are SolveGmres's own kernels, which
tests/test_gpu_gmres.py runs at that size."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.solver import ApplicationException, _ptr
from conjugategradient_amd.ssor import ConjugateGradientSsorGpu
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_amg_host import Hierarchy, csr_of
from tests.test_bicgstab_host import MAX_IT, nonsymmetric_tridiagonal, numpy_true_residual
from tests.test_bicgstab_mg_host import hierarchy, level, system
from tests.test_gmres_host import system as gmres_system
from tests.test_gmres_mg_host import HARD, OBSERVED, fgmres_oracle, hard_hierarchy, hard_system, run
from tests.test_gpu_bicgstab_mg import _maxnz, assert_equal_runs, build, tolerance
from tests.test_gs_host import GsHierarchy
from tests.test_sreduce_host import with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
WHO = "SolveGmresMg"
NONFINITE = ("the first residual is zero or not finite, or an Arnoldi step left no next direction and no column (A singular on the Krylov space, "
             "or a value that is not finite)")
# (system, maps, source) of tests/test_bicgstab_mg_host.py: "box" is MgSetup, "agg" MgSetupAggregation; "sym" is the hierarchy of
# problems.symmetric_part, a second object handed over through hierarchy=
TABLE_CASES = ([("convdiff12x10x8", maps, "own") for maps in ("box", "agg")] +
               [(name, maps, source) for name in ("convdiff16strong", "upwind16") for maps in ("box", "agg") for source in ("own", "sym")])
# m = 1: a restart at every step; 2: many restarts; 9: more than 8 columns, two x launches; 32: no restart
MS = (1, 2, 9, 32)
M, ORTH = 9, 2
CORE = [(c, m, ORTH) for c in TABLE_CASES for m in MS] + [(c, M, 1) for c in TABLE_CASES]
MAIN = ("convdiff16strong", "box", "own")


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def result_of(cg, messages=()):
    cg.Read()
    return dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual,
                status=cg.status, trace=cg.trace, messages=list(messages))


def finish(cg, m, orth, other=None):
    """SolveGmres() and everything read back; an iteration cap that was hit or a breakdown is a result here, not an exception."""
    with library_messages() as said:
        try:
            cg.SolveGmres(trace=True, hierarchy=other, m=m, orth=orth)
        except ApplicationException:
            assert cg.status == _lib.MAXIT_EXCEEDED
        except _lib.MgcgError:
            assert cg.status == _lib.NONFINITE
    return result_of(cg, said)


def solve(s, maps, source, m, orth, rule, tol, prepare=None, aggregates=None, **kw):
    """One solve through the class method.  prepare(cg): after Initialize()."""
    cg = build(s, maps, tol=tol, rule=rule, aggregates=aggregates, **kw)
    other = build(problems.symmetric_part(s), maps, rule=rule) if source == "sym" else None
    if prepare is not None:
        prepare(cg)
    out = finish(cg, m, orth, other)
    cg.Dispose()
    if other is not None:
        other.Dispose()
    return out


def c_call(cg, mg, m, orth, rule, tol, min_it, max_it, cap):
    """SolveGmresMg itself on the object's vectors, with a trace of `cap` entries."""
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(float("nan"))
    tr = np.zeros(max(cap, 1))
    L = _lib.lib()
    st = L.SolveGmresMg(cg.cublas, cg.cusparse, cg.matDescr, mg, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                        cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, cg.vectorWork.Ptr, m, orth,
                        int(cg.A.RowOffsets[cg.Count]), cg.Count, tol, min_it, max_it, rule, C.byref(it), C.byref(res), C.byref(true),
                        _ptr(tr) if cap else None, cap)
    message = _lib.last_error()
    L.MgcgClearLastError()
    cg.Read()
    return dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=it.value, residual=res.value, true_residual=true.value, status=st,
                trace=tr[: min(it.value + 1, cap)].copy(), message=message)


def main_case():
    name, maps, source = MAIN
    return system(name), hierarchy(name, maps, source).apply, name, maps, source


# --------------------------------------------------------------------------- 1. bit equality with the yardstick
@pytest.mark.parametrize("case,m,orth", CORE, ids=[f"{c[0]}-{c[1]}-{c[2]}-m{m}-orth{o}" for c, m, o in CORE])
def test_solve_equals_the_yardstick_bit_for_bit(dot_order, case, m, orth):
    name, maps, source = case
    s = system(name)
    ref = run(name, "randn", maps, source, m, orth)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, maps, source, m, orth, _lib.RULE_CSHARP, level(s))
    print(case, m, orth, "steps", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"], "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


_odd = {}


def _pairs_maps(n):
    """Rows 2k and 2k + 1 in one aggregate, twice: an odd level keeps its last row alone (675 -> 338 -> 169 rows)."""
    m0 = (np.arange(n) // 2).astype(np.int32)
    return [m0, (np.arange(int(m0.max()) + 1) // 2).astype(np.int32)]


ODD_CAP = 40                                                                       # one restart with m = 32, four with m = 9


def odd_case(pairs):
    """15 x 15 x 3, c = (5, 5, 5): 675 rows, odd -- the pair tail -- with odd plane sizes, through the aggregation class: the library's
    matching, which on this matrix finds no mutual picks and leaves ONE level (nuCoarse sweeps), or the caller's pairs (three levels)."""
    if pairs not in _odd:
        s, _ = gmres_system("convdiff15x15x3", "randn")
        _odd[pairs] = (s, Hierarchy(*csr_of(s), maps=_pairs_maps(s.Count)) if pairs else Hierarchy(*csr_of(s)))
    return _odd[pairs]


@pytest.mark.parametrize("m,orth,pairs", [(m, ORTH, False) for m in MS] + [(M, 1, False), (M, ORTH, True), (2, 1, True)])
def test_an_odd_row_count_through_the_aggregation_hierarchy(dot_order, m, orth, pairs):
    """At cell Peclet number 5 Jacobi sweeps are a poor map: no m brings this system to a relative 1e-8 within 3000 steps, in the
    yardstick either.  Bit equality does not need convergence: the runs are capped at ODD_CAP steps and end MGCG_MAXIT_EXCEEDED alike."""
    s, H = odd_case(pairs)
    ref = fgmres_oracle(s, m, orth, H.apply, _lib.RULE_CSHARP, level(s), max_it=ODD_CAP)
    print("15x15x3", m, orth, "residual", ref["residual"] / level(s), "x the level, rows per level", [len(L["ro"]) - 1 for L in H.levels])
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == ODD_CAP + 1 and np.isfinite(ref["x"]).all()
    got = solve(s, None if pairs else "agg", "own", m, orth, _lib.RULE_CSHARP, level(s), max_it=ODD_CAP, aggregates=_pairs_maps(s.Count) if pairs else None)
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 2. rules, start, minimum, cap, trace, sizes
@pytest.mark.parametrize("rule", RULES)
def test_the_four_rules_from_a_nonzero_guess(dot_order, rule):
    s, minv, name, maps, source = main_case()
    tol = tolerance(s, rule)
    start = with_b(s, s.b, "x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    ref = fgmres_oracle(start, M, ORTH, minv, rule, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] > M
    assert_equal_runs(solve(start, maps, source, M, ORTH, rule, tol), ref)


def test_min_iteration_beyond_convergence(dot_order):
    s, minv, name, maps, source = main_case()
    free = run(name, "randn", maps, source, M, ORTH, rel=1e-6)
    held = run(name, "randn", maps, source, M, ORTH, rel=1e-6, min_it=free["iteration"] + 5)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    assert_equal_runs(solve(s, maps, source, M, ORTH, _lib.RULE_CSHARP, level(s, 1e-6), min_it=free["iteration"] + 5), held)


@pytest.mark.parametrize("cap", [9, 12, 8])
def test_iteration_cap_equals_the_yardstick(dot_order, cap):
    """The last step at j = 0 behind a restart (cap 9), in mid-cycle (12) and at a cycle's last step (8): x is closed once."""
    s, minv, name, maps, source = main_case()
    ref = fgmres_oracle(s, M, ORTH, minv, _lib.RULE_CSHARP, 0.0, max_it=cap)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == cap + 1
    got = solve(s, maps, source, M, ORTH, _lib.RULE_CSHARP, 0.0, max_it=cap)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message(WHO, got, cap)]


def test_a_short_trace_and_the_class_method_gives_the_c_calls_result(dot_order):
    s, minv, name, maps, source = main_case()
    ref = dict(run(name, "randn", maps, source, M, ORTH))
    assert ref["iteration"] + 1 > 5
    cg = build(s, maps, tol=level(s))
    by_method = finish(cg, M, ORTH)
    assert_equal_runs(by_method, ref)
    cg.vectorX.CopyFrom(s.x, s.Count)
    whole = c_call(cg, cg.mg, M, ORTH, _lib.RULE_CSHARP, level(s), 0, MAX_IT, MAX_IT + 8)
    assert whole["message"] == ""
    assert_equal_runs(whole, by_method)
    cg.vectorX.CopyFrom(s.x, s.Count)
    short = c_call(cg, cg.mg, M, ORTH, _lib.RULE_CSHARP, level(s), 0, MAX_IT, 5)
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(short, ref)
    cg.Dispose()


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_tiny_systems_with_a_one_level_hierarchy(dot_order, n):
    """Fewer rows than a workgroup, than a 16-byte pair, than m: the Krylov space is exhausted inside the first cycle (hn = 0 at n = 1)."""
    s = nonsymmetric_tridiagonal(n)
    minv = Hierarchy(*csr_of(s), maps=[]).apply
    for m in (2, 32):
        ref = fgmres_oracle(s, m, ORTH, minv, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
        assert ref["status"] == _lib.OK
        assert_equal_runs(solve(s, None, "own", m, ORTH, _lib.RULE_CSHARP, level(s), aggregates=[]), ref)


# --------------------------------------------------------------------------- 3. matrix forms, work space, corner cases, other cycles
def test_every_compression_mode_gives_the_mode_0_bits(dot_order):
    s, minv, name, maps, source = main_case()
    runs = [solve(s, maps, source, M, ORTH, _lib.RULE_CSHARP, level(s), compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], run(name, "randn", maps, source, M, ORTH))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("m", [2, M])
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, m):
    """NaN in all 2 m + 1 slices of the work vector and in p, Ap and r: a cycle enqueued behind the stop leaves its slice as it was."""
    s, minv, name, maps, source = main_case()
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        size = (2 * m + 1) * (s.Count + (s.Count & 1))
        cg.vectorWork, cg._work_size = dvec(np.full(size, np.nan)), size
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR):
            v.CopyFrom(nan, s.Count)

    assert_equal_runs(solve(s, maps, source, m, ORTH, _lib.RULE_CSHARP, level(s), prepare=prepare), run(name, "randn", maps, source, m, ORTH))


def test_a_zero_right_hand_side_gives_nonfinite(dot_order):
    s, minv, name, maps, source = main_case()
    zero = with_b(s, np.zeros(s.Count), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = fgmres_oracle(zero, M, ORTH, minv, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        got = solve(zero, maps, source, M, ORTH, rule, 1e-12)
        assert_equal_runs(got, ref)
        assert got["messages"] == [nonfinite_message(WHO, got, NONFINITE)]


def test_a_gauss_seidel_smoothed_aggregation_hierarchy(dot_order):
    s = system("convdiff16strong")
    H = GsHierarchy(*csr_of(s))
    ref = fgmres_oracle(s, M, ORTH, H.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, MAX_IT, level(s), smoother="gs").load(s)
    cg.Initialize()
    got = finish(cg, M, ORTH)
    cg.Dispose()
    assert_equal_runs(got, ref)


def test_the_one_level_ssor_class(dot_order):
    s = system("upwind16")
    H = GsHierarchy(*csr_of(s), maps=[], nuCoarse=2, omega=1.0)
    ref = fgmres_oracle(s, M, ORTH, H.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    cg = ConjugateGradientSsorGpu(s.Count, _maxnz(s), 0, MAX_IT, level(s)).load(s)
    cg.Initialize()
    got = finish(cg, M, ORTH)
    cg.Dispose()
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 4. default mode
@pytest.mark.parametrize("m,orth", [(20, 2), (9, 1)])
@pytest.mark.parametrize("case", TABLE_CASES, ids=["-".join(c) for c in TABLE_CASES])
def test_default_dot_order_solves_every_case(case, m, orth):
    name, maps, source = case
    s = system(name)
    tol = level(s)
    got = solve(s, maps, source, m, orth, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, got["x"])
    print(case, m, orth, "steps", got["iteration"], "yardstick", run(name, "randn", maps, source, m, orth)["iteration"] if m == 20 else "-", "estimate", got["residual"],
          "TrueResidual", got["true_residual"], "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == _lib.OK
    assert true <= 1.001 * tol
    assert abs(got["true_residual"] - true) <= 1e-10 * true


# --------------------------------------------------------------------------- 5. the capability
def test_gmres_converges_where_preconditioned_bicgstab_does_not():
    """16^3, c = (2, 2, 2), the box hierarchy of the matrix itself (default summation order)."""
    name, rhs = "convdiff16c2", "randn"
    s = hard_system(name, rhs)
    tol = level(s)
    cap = OBSERVED[name, rhs] * 3 // 2
    cg = build(s, "box", tol=tol, max_it=1000)
    try:
        cg.SolveBicgstab()
    except (_lib.MgcgError, ApplicationException):
        pass
    print("SolveBicgstabMg: status", cg.status, "at body", cg.Iteration, "TrueResidual", cg.TrueResidual / tol, "x the level")
    assert cg.status != _lib.OK
    cg.Dispose()
    got = solve(s, "box", "own", 20, ORTH, _lib.RULE_CSHARP, tol, max_it=cap)
    true = numpy_true_residual(s, got["x"])
    print("SolveGmresMg(20):", got["iteration"], "steps (cap", cap, "), TrueResidual", got["true_residual"] / tol, "numpy", true / tol, "x the level")
    assert got["status"] == _lib.OK and true <= 1.001 * tol


# --------------------------------------------------------------------------- 6. the object
def test_a_second_solve_a_raised_m_and_another_objects_hierarchy(dot_order):
    s, minv, name, maps, source = main_case()
    stride = s.Count + (s.Count & 1)
    cg = build(s, maps, tol=level(s))
    assert getattr(cg, "vectorWork", None) is None
    first = finish(cg, 2, ORTH)
    assert_equal_runs(first, run(name, "randn", maps, source, 2, ORTH))
    assert cg._work_size == 5 * stride
    cg.vectorX.CopyFrom(s.x, s.Count)
    assert_equal_runs(finish(cg, 2, ORTH), first)                          # a second solve
    cg.vectorX.CopyFrom(s.x, s.Count)
    assert_equal_runs(finish(cg, M, ORTH), run(name, "randn", maps, source, M, ORTH))     # m raised on the live object
    assert cg._work_size == (2 * M + 1) * stride
    other = build(problems.symmetric_part(s), maps)
    cg.vectorX.CopyFrom(s.x, s.Count)
    assert_equal_runs(finish(cg, M, ORTH, other), run(name, "randn", maps, "sym", M, ORTH))   # the hierarchy of another object
    assert cg._work_size == (2 * M + 1) * stride
    other.Dispose()
    cg.Dispose()
    assert cg.vectorWork is None


def test_refusals_leave_the_object_able_to_solve(dot_order):
    s, minv, name, maps, source = main_case()
    cg = build(s, maps, tol=level(s))
    stride = s.Count + (s.Count & 1)
    assert_equal_runs(finish(cg, 2, ORTH), run(name, "randn", maps, source, 2, ORTH))
    cg.vectorX.CopyFrom(s.x, s.Count)
    short = c_call(cg, cg.mg, M, ORTH, _lib.RULE_CSHARP, level(s), 0, MAX_IT, 0)      # the work vector is m = 2's
    assert short["status"] == _lib.ERROR and np.array_equal(short["x"], s.x)
    assert short["message"] == (f"SolveGmresMg: the work vector holds {5 * stride} entries, m = {M} needs {(2 * M + 1) * stride} "
                                f"({2 * M + 1} slices of {stride}: the matrix has {s.Count} rows)")
    small = build(problems.convection_diffusion(8, 8, 8, (0.5, 0.25, 0.0)), "box")
    with pytest.raises(_lib.MgcgError, match="SolveGmresMg: the hierarchy has 512 rows on level 0, the matrix has 4096"):
        cg.SolveGmres(hierarchy=small)
    assert cg.status == _lib.ERROR
    with pytest.raises(_lib.MgcgError, match="m = 33, must be 1 .. 32"):
        cg.SolveGmres(m=33)
    with pytest.raises(_lib.MgcgError, match="orth = 3, must be 1 or 2"):
        cg.SolveGmres(orth=3)
    cg.Read()
    assert np.array_equal(cg.x, s.x)                                       # nothing was enqueued
    # ... and both objects stay usable: the refused one solves with its own hierarchy
    assert_equal_runs(finish(cg, M, ORTH), run(name, "randn", maps, source, M, ORTH))
    small.Dispose()
    cg.Dispose()
