"""V-cycle-preconditioned BiCGStab on the GPU (SolveBicgstabMg, ConjugateGradientMgGpu.SolveBicgstab, inherited by ConjugateGradientAmgGpu).

The reference for every comparison is ``pbicgstab_oracle`` with ``Hierarchy.apply`` as M^-1 (tests/test_bicgstab_mg_host.py,
tests/test_amg_host.py): the header's loop and the cycle in numpy with serial sums.  Under dot_order = 1 the HIP loop is a fixed sequence of
IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of x and r must EQUAL it.  In the default mode the summation
order differs, and with it the iteration count, so only the solution's quality is asserted: the true residual within 1.001 x the stop
level, which test_bicgstab_mg_host.py shows to be safe on these inputs.

The hierarchies are built from nonsymmetric matrices, which no other test does: section 1 checks that every set-up path used here -- MgSetup
in 3-D and 2-D, MgSetupAggregation, MgSetupAggregates -- gives the level matrices and the cycle of the numpy yardstick on them."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException, VectorDouble, _ptr
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_amg_host import Hierarchy, csr_of
from tests.test_bicgstab_host import MAX_IT, numpy_true_residual
from tests.test_bicgstab_mg_host import hierarchy, level, pbicgstab_oracle, run, source_matrix, system
from tests.test_gpu_amg import _assert_apply_equals, _assert_equal_hierarchies
from tests.test_sreduce_host import with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
WHO = "SolveBicgstabMg"
NONFINITE = "the first residual is zero or not finite, or the recurrence broke down (rhat.v, omega or rhat.r zero, or a value that is not finite)"
WORK = ("vectorV", "vectorS", "vectorT", "vectorRhat")
# case -> (system, maps, source) of tests/test_bicgstab_mg_host.py: "box" is MgSetup (the 2-D hierarchy on 32^2), "agg" MgSetupAggregation; "sym" is
# the hierarchy of problems.symmetric_part, a second object handed over through hierarchy=
CASES = {
    "convdiff16-own": ("convdiff16", "box", "own"),
    "convdiff16-sym": ("convdiff16", "box", "sym"),
    "upwind16-aggregation": ("upwind16", "agg", "own"),
    "convdiff32x32-own": ("convdiff32x32", "box", "own"),
    "convdiff32x32-aggregation": ("convdiff32x32", "agg", "own"),                     # a matching that coarsens a nonsymmetric matrix: 3 levels
    "poisson16-own": ("poisson16", "box", "own"),
}
MAIN = "convdiff16-own"


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def _maxnz(s):
    return int(np.diff(s.RowOffsets).max())


def build(s, maps, min_it=0, max_it=MAX_IT, tol=1e-8, rule=_lib.RULE_CSHARP, compression=None, aggregates=None):
    """The multigrid object of a system, initialised: MgSetup on its grid ("box"), MgSetupAggregation ("agg") or MgSetupAggregates."""
    if aggregates is not None:
        cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), min_it, max_it, tol, aggregates=aggregates, rule=rule).load(s)
    elif maps == "box":
        cg = ConjugateGradientMgGpu(s.Count, _maxnz(s), min_it, max_it, tol, s.grid, rule=rule).load(s)
    else:
        cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), min_it, max_it, tol, rule=rule).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    return cg


def result_of(cg, messages=()):
    cg.Read()
    return dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual,
                status=cg.status, trace=cg.trace, messages=list(messages))


def solve(s, maps, source, rule, tol, prepare=None, aggregates=None, **kw):
    """One solve through the class method; an iteration cap that was hit or a breakdown is a result here, not an exception.
    prepare(cg): after Initialize()."""
    cg = build(s, maps, tol=tol, rule=rule, aggregates=aggregates, **kw)
    other = None
    if source == "sym":
        other = build(problems.symmetric_part(s), maps, rule=rule)
    if prepare is not None:
        prepare(cg)
    with library_messages() as said:
        try:
            cg.SolveBicgstab(trace=True, hierarchy=other)
        except ApplicationException:
            assert cg.status == _lib.MAXIT_EXCEEDED
        except _lib.MgcgError:
            assert cg.status == _lib.NONFINITE
    out = result_of(cg, said)
    cg.Dispose()
    if other is not None:
        other.Dispose()
    return out


def c_call(cg, mg, rule, tol, min_it, max_it, cap):
    """SolveBicgstabMg itself on the object's vectors, with a trace of `cap` entries."""
    for name in WORK:
        if getattr(cg, name, None) is None:
            setattr(cg, name, VectorDouble(cg.Count))
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(float("nan"))
    tr = np.zeros(max(cap, 1))
    L = _lib.lib()
    st = L.SolveBicgstabMg(cg.cublas, cg.cusparse, cg.matDescr, mg, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                           cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr,
                           cg.vectorV.Ptr, cg.vectorS.Ptr, cg.vectorT.Ptr, cg.vectorRhat.Ptr, int(cg.A.RowOffsets[cg.Count]), cg.Count,
                           tol, min_it, max_it, rule, C.byref(it), C.byref(res), C.byref(true), _ptr(tr) if cap else None, cap)
    message = _lib.last_error()
    L.MgcgClearLastError()
    cg.Read()
    return dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=it.value, residual=res.value, true_residual=true.value, status=st,
                trace=tr[: min(it.value + 1, cap)].copy(), message=message)


def tolerance(s, rule, rel=1e-8):
    assert not s.x.any()
    return rel if rule == _lib.RULE_VIENNACL else level(s, rel)


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


def main_case():
    name, maps, source = CASES[MAIN]
    return system(name), hierarchy(name, maps, source).apply, name, maps, source


# --------------------------------------------------------------------------- 1. the set-up on nonsymmetric input
def _levels_of(H):
    return [(L["e"], L["c"], L["ro"], L["dinv"]) for L in H.levels]


@pytest.mark.parametrize("name,maps,levels", [("convdiff16", "box", 3), ("upwind16", "box", 3), ("convdiff32x32", "box", 3), ("convdiff12x10x8", "box", 2),
                                              ("convdiff16", "agg", 2), ("convdiff32x32", "agg", 3), ("upwind16", "agg", 1)])
def test_the_setup_of_a_nonsymmetric_matrix_equals_the_yardstick(name, maps, levels):
    """Level matrices, D^-1, the maps of the matching and one cycle, compared as tests/test_gpu_amg.py compares them.  The matching pairs
    rows on mutual picks: on the upwind stencil every row's heaviest coupling points upstream, nobody is picked back, and the hierarchy is
    one level -- nuCoarse Jacobi sweeps -- in the yardstick and in the library alike."""
    s = system(name)
    H = hierarchy(name, maps, "own")
    a = s.to_scipy()
    assert (a != a.T).nnz > 0 and len(H.levels) == levels
    cg = build(s, maps)
    print(f"{name} {maps}: rows per level {[len(L['ro']) - 1 for L in H.levels]}")
    _assert_equal_hierarchies(cg, _levels_of(H))
    if maps == "agg":
        for l, L in enumerate(H.levels[:-1]):
            assert np.array_equal(cg.level_aggregates(l), L["map"]), l
    _assert_apply_equals(cg, H, np.random.default_rng(5).standard_normal(s.Count), f"{name} {maps}")
    cg.Dispose()


# --------------------------------------------------------------------------- 2. bit equality with the yardstick
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", list(CASES))
def test_solve_equals_the_yardstick_bit_for_bit(dot_order, case, rule):
    name, maps, source = CASES[case]
    s = system(name)
    ref = run(name, "randn", maps, source, rule)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, maps, source, rule, tolerance(s, rule))
    print(case, rule, "bodies", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"], "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 3. start, minimum, cap, trace, sizes
def test_a_nonzero_initial_guess(dot_order):
    s, minv, name, maps, source = main_case()
    start = with_b(s, s.b, "convdiff16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    ref = pbicgstab_oracle(start, minv, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, maps, source, _lib.RULE_CSHARP, level(s)), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, maps, source, _lib.RULE_SIMPLE, level(s)), run(name, "randn", maps, source, _lib.RULE_SIMPLE))


def test_min_iteration_beyond_convergence(dot_order):
    s, minv, name, maps, source = main_case()
    free = run(name, "randn", maps, source, rel=1e-6)
    held = run(name, "randn", maps, source, rel=1e-6, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, maps, source, _lib.RULE_CSHARP, level(s, 1e-6), min_it=free["iteration"] + 6), held)


def test_the_iteration_cap_raises_and_equals_the_yardstick(dot_order):
    s, minv, name, maps, source = main_case()
    ref = pbicgstab_oracle(s, minv, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(s, maps, source, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message(WHO, got, 3)]
    cg = build(s, maps, max_it=3, tol=0.0)
    with pytest.raises(ApplicationException):
        cg.SolveBicgstab()
    assert cg.status == _lib.MAXIT_EXCEEDED and np.array_equal(result_of(cg)["x"], ref["x"])
    cg.Dispose()


def test_a_trace_shorter_than_the_run_and_the_class_method_gives_the_c_calls_result(dot_order):
    s, minv, name, maps, source = main_case()
    ref = dict(run(name, "randn", maps, source))
    assert ref["iteration"] + 1 > 5
    cg = build(s, maps, tol=level(s))
    cg.SolveBicgstab(trace=True)
    by_method = result_of(cg)
    assert_equal_runs(by_method, ref)
    cg.vectorX.CopyFrom(s.x, s.Count)
    whole = c_call(cg, cg.mg, _lib.RULE_CSHARP, level(s), 0, MAX_IT, MAX_IT + 8)
    assert whole["message"] == ""
    assert_equal_runs(whole, by_method)
    cg.vectorX.CopyFrom(s.x, s.Count)
    short = c_call(cg, cg.mg, _lib.RULE_CSHARP, level(s), 0, MAX_IT, 5)
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(short, ref)
    cg.Dispose()


def _pairs(n):
    """Rows 2k and 2k + 1 in one aggregate: an odd level keeps its last row alone."""
    return (np.arange(n) // 2).astype(np.int32)


@pytest.mark.parametrize("dims", [(15, 15, 1), (15, 15, 3)])
def test_an_odd_row_count_through_the_callers_aggregates(dot_order, dims):
    """225 and 675 rows: the odd tail element of the 16-byte path runs, in one workgroup and in several; the levels hold 113 and 57 (338
    and 169) rows, odd again."""
    s = problems.convection_diffusion(*dims, (0.5, 0.25, 0.1))
    s = with_b(s, np.random.default_rng(3).standard_normal(s.Count), "odd")
    m0 = _pairs(s.Count)
    maps = [m0, _pairs(int(m0.max()) + 1)]
    H = Hierarchy(*csr_of(s), maps=maps)
    ref = pbicgstab_oracle(s, H.apply, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    plain_count = pbicgstab_oracle(s, lambda v: v, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)["iteration"]
    print(dims, "bodies", ref["iteration"], "plain", plain_count)
    assert ref["status"] == _lib.OK and 3 <= ref["iteration"] < plain_count
    cg = build(s, None, aggregates=maps)
    _assert_equal_hierarchies(cg, _levels_of(H))
    _assert_apply_equals(cg, H, np.random.default_rng(5).standard_normal(s.Count), f"pairs {dims}")
    cg.Dispose()
    assert_equal_runs(solve(s, None, "own", _lib.RULE_CSHARP, level(s), aggregates=maps), ref)


# --------------------------------------------------------------------------- 4. default mode
@pytest.mark.parametrize("case", list(CASES))
def test_default_dot_order_solves_every_case(case):
    name, maps, source = CASES[case]
    s = system(name)
    tol = level(s)
    got = solve(s, maps, source, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, got["x"])
    print(case, "bodies", got["iteration"], "yardstick", run(name, "randn", maps, source)["iteration"], "recurrence", got["residual"],
          "TrueResidual", got["true_residual"], "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == _lib.OK
    assert true <= 1.001 * tol
    assert abs(got["true_residual"] - true) <= 1e-10 * true


# --------------------------------------------------------------------------- 5. matrix forms, work space, corner cases, refusals
def test_every_compression_mode_gives_the_mode_0_bits(dot_order):
    s, minv, name, maps, source = main_case()
    runs = [solve(s, maps, source, _lib.RULE_CSHARP, level(s), compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], run(name, "randn", maps, source))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order):
    """NaN in all seven work vectors."""
    s, minv, name, maps, source = main_case()
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR):
            v.CopyFrom(nan, s.Count)
        for work in WORK:
            setattr(cg, work, dvec(nan))

    assert_equal_runs(solve(s, maps, source, _lib.RULE_CSHARP, level(s), prepare=prepare), run(name, "randn", maps, source))


def test_a_zero_right_hand_side_gives_nonfinite(dot_order):
    s, minv, name, maps, source = main_case()
    zero = with_b(s, np.zeros(s.Count), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = pbicgstab_oracle(zero, minv, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        got = solve(zero, maps, source, rule, 1e-12)
        assert_equal_runs(got, ref)
        assert got["messages"] == [nonfinite_message(WHO, got, NONFINITE)]


def test_a_hierarchy_of_another_size_is_refused_with_the_row_counts(dot_order):
    s, minv, name, maps, source = main_case()
    cg = build(s, maps, tol=level(s))
    small = build(problems.convection_diffusion(8, 8, 8, (0.5, 0.25, 0.0)), "box")
    with pytest.raises(_lib.MgcgError, match="SolveBicgstabMg: the hierarchy has 512 rows on level 0, the matrix has 4096"):
        cg.SolveBicgstab(hierarchy=small)
    assert cg.status == _lib.ERROR
    cg.Read()
    assert np.array_equal(cg.x, s.x)                        # nothing was enqueued
    # ... and both objects stay usable: the refused one solves with its own hierarchy
    cg.SolveBicgstab(trace=True)
    assert_equal_runs(result_of(cg), run(name, "randn", maps, source))
    small.Dispose()
    cg.Dispose()


def test_dispose_frees_the_work_vectors(dot_order):
    s, minv, name, maps, source = main_case()
    cg = build(s, maps, tol=level(s))
    assert all(getattr(cg, work, None) is None for work in WORK)
    cg.SolveBicgstab()
    assert all(getattr(cg, work).size >= s.Count for work in WORK)
    cg.Dispose()
    assert all(getattr(cg, work) is None for work in WORK)
