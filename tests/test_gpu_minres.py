"""MINRES on the GPU (SolveMinres, SolveMinresParallel, minres.MinimalResidualGpu, ConjugateGradientRankGpu.SolveMinres).

The reference for every comparison is ``minres_oracle`` (tests/test_minres_host.py): the header's loop in numpy with serial sums.
Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, residual, TrueResidual, trace and ALL of
x and r must EQUAL it; in the default mode only the summation order of the sums (and of long rows) differs."""
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.minres import MinimalResidualGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_gpu_jacobi import run_ranks
from tests.test_minres_host import CASES, indefinite2, minres_oracle, numpy_true_residual, singular2, system
from tests.test_sreduce_host import tridiagonal, with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
MAX_IT = 3000
# every (system, shift) under the four 2-norm rules; the longest run (viennacl4000, shift 60: about 450 iterations) under one rule only
RULE_CASES = [(n, sh, r) for n, sh in CASES for r in RULES if (n, sh) != ("viennacl4000", 60.0) or r == _lib.RULE_CSHARP]
_oracles = {}
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_minres)
NONFINITE = ("the first residual is zero or not finite, or the rotation broke down (A - shift I singular on the Krylov space, or a value that is not "
             "finite)")


def reference(name, shift, rule, tol, parts=None, **kw):
    """The oracle's run, computed once per case and shared (nothing changes it)."""
    key = (name, shift, rule, tol, None if parts is None else tuple(parts), tuple(sorted(kw.items())))
    if key not in _oracles:
        _oracles[key] = minres_oracle(system(name), shift, rule, tol, parts=parts, **{"max_it": MAX_IT, **kw})
    return _oracles[key]


def tolerance(s, rule, rel=1e-8):
    """The relative rule: rel; the absolute rules: rel of the first residual's 2-norm (every system here starts from x = 0: r0 = b)."""
    assert not s.x.any()
    return rel if rule == _lib.RULE_VIENNACL else rel * float(np.linalg.norm(s.b))


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def solve(s, shift, rule, tol, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None):
    """One solve through the Python class; an iteration cap that was hit or a breakdown is a result here, not an exception.
    prepare(cg): after Initialize()."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = MinimalResidualGpu(s.Count, maxnz, min_it, max_it, tol, rule=rule, shift=shift).load(s)
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
@pytest.mark.parametrize("which,shift,rule", RULE_CASES)
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, shift, rule):
    s = system(which)
    tol = tolerance(s, rule)
    ref = reference(which, shift, rule, tol)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, shift, rule, tol)
    print(which, shift, rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"],
          "true", got["true_residual"], ref["true_residual"])
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 2. sizes, start, minimum, cap, trace
@pytest.mark.parametrize("shift", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 2, 7, 300, 257 * 3])
def test_small_and_odd_sizes_equal_the_oracle(dot_order, n, shift):
    """Less than a workgroup, no multiple of 256 or of the 16-byte access, more than one workgroup; n = 1 ends by betan == 0."""
    s, _ = tridiagonal(n)
    tol = 1e-10 * float(np.linalg.norm(s.b))
    ref = minres_oracle(s, shift, _lib.RULE_CSHARP, tol)
    assert ref["status"] == _lib.OK
    assert_equal_runs(solve(s, shift, _lib.RULE_CSHARP, tol), ref)


def test_a_nonzero_initial_guess(dot_order):
    s = system("poisson16")
    start = with_b(s, s.b, "poisson16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = minres_oracle(start, 0.5, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, 0.5, _lib.RULE_CSHARP, tol), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, 0.5, _lib.RULE_SIMPLE, tol), reference("poisson16", 0.5, _lib.RULE_SIMPLE, tol))


def test_min_iteration_beyond_convergence(dot_order):
    s, _ = tridiagonal(300)
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = minres_oracle(s, 0.01, _lib.RULE_CSHARP, tol)
    held = minres_oracle(s, 0.01, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, 0.01, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6), held)


def test_iteration_cap_equals_the_oracle(dot_order):
    ref = reference("poisson16", 0.5, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(system("poisson16"), 0.5, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message("SolveMinres", got, 3)]         # "SolveMinres: did not converge: iteration 4 exceeded maxIteration 3 (residual ...)"


def test_a_trace_shorter_than_the_run(dot_order):
    s = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = dict(reference("poisson16", 0.5, _lib.RULE_CSHARP, tol))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, 0.5, _lib.RULE_CSHARP, tol, trace_capacity=5), ref)


# --------------------------------------------------------------------------- 3. / 4. default mode
@pytest.mark.parametrize("which", [n for n, sh in CASES if sh == 0.0])
def test_default_dot_order_stays_within_1e_10_of_the_oracle(which):
    """shift 0, tolerance 1e-13 of || b ||, so that the one iteration the two runs may differ by moves x by far less than the bound: the
    oracle itself moves by at most 9e-16 (2-norm, relative; 6.6e-16, 7.9e-16 and 8.9e-16) on these systems when its serial sums are
    replaced by numpy's pairwise ones, measured at this tolerance; its iteration counts (88, 76, 130) do not move."""
    s = system(which)
    tol = 1e-13 * float(np.linalg.norm(s.b))
    ref = reference(which, 0.0, _lib.RULE_CSHARP, tol)
    got = solve(s, 0.0, _lib.RULE_CSHARP, tol)
    distance = float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    print(which, "iterations", got["iteration"], ref["iteration"], "distance", distance)
    assert got["status"] == ref["status"] == _lib.OK
    assert abs(got["iteration"] - ref["iteration"]) <= 1
    assert distance <= 1e-10


@pytest.mark.parametrize("which,shift", [(n, sh) for n, sh in CASES if sh != 0.0])
def test_default_dot_order_solves_the_indefinite_systems(which, shift):
    """An indefinite Lanczos run is sensitive to the order of its sums: the oracle's own count moves 447 -> 432 on viennacl4000, shift 60,
    between serial and pairwise sums with one N(0,1) right-hand side (451 -> 450 with the one used here), and by 0 on the other systems.  So the counts are not compared tightly: status OK, the numpy true
    residual of x at most 2 x the stop level (the oracle's is <= 1.0 x; the factor 2 is for the drift of phibar under another summation
    order), the count within 10 % of the oracle's (twice the 3.4 % measured on that system, rounded up)."""
    s = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = reference(which, shift, _lib.RULE_CSHARP, tol)
    got = solve(s, shift, _lib.RULE_CSHARP, tol)
    true = numpy_true_residual(s, shift, got["x"])
    print(which, shift, "iterations", got["iteration"], ref["iteration"], "recurrence", got["residual"], "TrueResidual", got["true_residual"],
          "numpy true residual", true, "=", true / tol, "x the stop level")
    assert got["status"] == ref["status"] == _lib.OK
    assert true <= 2.0 * tol
    assert abs(got["iteration"] - ref["iteration"]) <= 0.1 * ref["iteration"]
    # what the call reports as the true residual is that figure, up to the rounding of the closing product (the bound of test_minres_host.py)
    m = int(np.diff(s.RowOffsets).max())
    absx = np.abs(got["x"])
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    scale = np.bincount(rows, weights=np.abs(s.Elements[: s.nnz]) * absx[s.ColumnIndeces[: s.nnz]], minlength=s.Count) + np.abs(s.b) + abs(shift) * absx
    assert abs(got["true_residual"] - true) <= (m + 2) * np.finfo(np.float64).eps * float(np.linalg.norm(scale))


# --------------------------------------------------------------------------- 5. - 8. matrix forms, work space, corner cases, the trace
def test_every_compression_mode_gives_the_mode_0_bits(dot_order):
    s = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, 0.5, _lib.RULE_CSHARP, tol, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], reference("poisson16", 0.5, _lib.RULE_CSHARP, tol))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order):
    """NaN in all five work vectors (q, the two Lanczos buffers, the two direction buffers)."""
    s = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR, cg.vectorW1, cg.vectorW2):
            v.CopyFrom(nan, s.Count)
        dvec(nan).Dispose()

    assert_equal_runs(solve(s, 0.5, _lib.RULE_CSHARP, tol, prepare=prepare), reference("poisson16", 0.5, _lib.RULE_CSHARP, tol))


def test_the_indefinite_2x2_matrix_is_solved(dot_order):
    s = indefinite2()
    ref = minres_oracle(s, 0.0, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.OK and numpy_true_residual(s, 0.0, ref["x"]) < 1e-12
    assert_equal_runs(solve(s, 0.0, _lib.RULE_CSHARP, 1e-12), ref)


def test_a_singular_shifted_matrix_gives_nonfinite_and_the_callers_x_back(dot_order):
    s = singular2()
    ref = minres_oracle(s, 1.0, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 1 and np.array_equal(ref["x"], s.x)
    got = solve(s, 1.0, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message("SolveMinres", got, NONFINITE)]


def test_a_zero_right_hand_side_gives_nonfinite(dot_order):
    s, _ = tridiagonal(50)
    zero = with_b(s, np.zeros(50), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = minres_oracle(zero, 0.01, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        assert_equal_runs(solve(zero, 0.01, rule, 1e-12), ref)


@pytest.mark.parametrize("serial", [False, True], ids=["default", "dot_order"])
def test_the_trace_read_back_never_increases(mgcg_env, serial):
    if serial:
        mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    for which, shift in (("poisson16", 0.5), ("random_spd5000", 1.5)):
        s = system(which)
        got = solve(s, shift, _lib.RULE_CSHARP, tolerance(s, _lib.RULE_CSHARP))
        assert got["status"] == _lib.OK and len(got["trace"]) == got["iteration"] + 1 >= 4
        assert (np.diff(got["trace"]) <= 0.0).all()


# --------------------------------------------------------------------------- 9. the streaming-hint form of the passes
STREAMING_ROWS = 3_000_001      # the smallest row count at which the passes take their streaming-hint form (n > 3 000 000); odd: the tail element runs
_streaming = {}


def test_streaming_hint_form_equals_the_oracle(dot_order):
    """Six forced bodies, tolerance 0, so that both sides stop at the iteration cap."""
    if "s" not in _streaming:
        _streaming["s"] = tridiagonal(STREAMING_ROWS)[0]
    s = _streaming["s"]
    ref = minres_oracle(s, 0.01, _lib.RULE_CSHARP, 0.0, max_it=5)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 6
    assert_equal_runs(solve(s, 0.01, _lib.RULE_CSHARP, 0.0, max_it=5), ref)


# --------------------------------------------------------------------------- 10. ranks
def _rank_solve(s, world, shift, rule, tol, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, max_it, tol, rank=rank, world=world, comm=comm, rule=rule, device=rank).load(s)
        cg.Initialize()
        cg.SolveMinres(trace=True, shift=shift)
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
@pytest.mark.parametrize("which,shift", [("poisson16", 0.5), ("random_spd5000", 1.5)])
def test_ranks_equal_the_oracle_with_its_sums_cut_at_their_rows(mgcg_env, dot_order, which, shift, world):
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    parts = problems.partition_offsets(s.Count, world)
    ref = reference(which, shift, _lib.RULE_CSHARP, tol, parts=parts)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    _assert_ranks_equal(_rank_solve(s, world, shift, _lib.RULE_CSHARP, tol), ref, parts)


def test_a_rank_without_rows_takes_part(mgcg_env, dot_order):
    world = 4
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = problems.mgcg_main(3, 160)                      # 3 rows over 4 ranks: offsets [0, 0, 0, 0, 3]
    parts = problems.partition_offsets(s.Count, world)
    assert parts == [0, 0, 0, 0, 3]
    ref = minres_oracle(s, 0.25, _lib.RULE_CSHARP, 1e-8, max_it=50, parts=parts)
    assert ref["status"] == _lib.OK
    res = _rank_solve(s, world, 0.25, _lib.RULE_CSHARP, 1e-8, max_it=50)
    assert [k["count"] for k in res] == [0, 0, 0, 3]
    _assert_ranks_equal(res, ref, parts)


def test_the_forced_several_ranks_path_on_one_rank_equals_the_one_rank_loop(mgcg_env, dot_order):
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
    s = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, MAX_IT, tol, rank=0, world=1, comm=comm, rule=_lib.RULE_CSHARP, device=0).load(s)
    cg.Initialize()
    cg.SolveMinres(trace=True, shift=0.5)
    cg.Read()
    r = np.zeros(s.Count)
    cg.vectorR.CopyTo(r, s.Count, 0)
    got = dict(x=cg.x.copy(), r=r, iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual, status=cg.status, trace=cg.trace)
    cg.Dispose()
    assert_equal_runs(got, reference("poisson16", 0.5, _lib.RULE_CSHARP, tol))
    L.MgcgCommDestroy(comm)
