"""Single-reduction CG on the GPU (SolveSingleReduce, SolveSingleReduceParallel, singlereduce.ConjugateGradientSingleReduceGpu,
ConjugateGradientRankGpu.SolveSingleReduce).

The reference for every comparison is ``sreduce_cg_oracle`` (tests/test_sreduce_host.py): the header's loop in numpy with serial sums.
Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and trace, iteration, residual, status and ALL of x and r must
EQUAL it; in the default mode only the summation order of the three sums (and of long rows) differs."""
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.singlereduce import ConjugateGradientSingleReduceGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import dvec, library_messages, maxit_message, nonfinite_message
from tests.test_gpu_jacobi import run_ranks
from tests.test_sreduce_host import diagonal_of, randn_b, sreduce_cg_oracle, tridiagonal, with_b

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
VARIANTS = [False, True]
MAX_IT = 3000

# random_spd's own b is A 1 = 1, an eigenvector (one body solves it): it gets the N(0,1) right-hand side
SYSTEMS = {
    "poisson16": lambda: problems.poisson(16, 16, 16),
    "viennacl4000": lambda: problems.viennacl_main(4000),
    "random_spd5000": lambda: randn_b(problems.random_spd(5000), "random_spd5000"),
}
_systems, _oracles = {}, {}
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_sreduce)
NONFINITE = "w.u or its corrected form is not finite and > 0, or alpha or the residual is not finite"


def system(name):
    if name not in _systems:
        s = SYSTEMS[name]()
        _systems[name] = (s, diagonal_of(s))
    return _systems[name]


def reference(name, rule, tol, jacobi, parts=None, **kw):
    """The oracle's run, computed once per case and shared (nothing changes it)."""
    key = (name, rule, tol, jacobi, None if parts is None else tuple(parts), tuple(sorted(kw.items())))
    if key not in _oracles:
        s, diag = system(name)
        _oracles[key] = sreduce_cg_oracle(s, rule, tol, jacobi=jacobi, diag=diag, parts=parts, **{"max_it": MAX_IT, **kw})
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


def solve(s, rule, tol, jacobi, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None):
    """One solve through the Python class; an iteration cap that was hit is a result here, not an exception.  prepare(cg): after Initialize()."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientSingleReduceGpu(s.Count, maxnz, min_it, max_it, tol, rule=rule, jacobi=jacobi).load(s)
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
    out = dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace, messages=list(said))
    cg.Dispose()
    return out


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert got["residual"] == ref["residual"] or (math.isnan(got["residual"]) and math.isnan(ref["residual"]))
    assert np.array_equal(got["trace"], ref["trace"], equal_nan=True)
    assert np.array_equal(got["x"], ref["x"])
    assert np.array_equal(got["r"], ref["r"])


# --------------------------------------------------------------------------- 1. bit equality with the oracle
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, jacobi, rule):
    s, _ = system(which)
    tol = tolerance(s, rule)
    ref = reference(which, rule, tol, jacobi)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, rule, tol, jacobi)
    print(which, jacobi, rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("n", [1, 7, 300, 257 * 3])
def test_small_and_odd_sizes_equal_the_oracle(dot_order, n, jacobi):
    """Less than a workgroup, no multiple of 256 or of the 16-byte access, more than one workgroup."""
    s, diag = tridiagonal(n)
    tol = 1e-10 * float(np.linalg.norm(s.b))
    ref = sreduce_cg_oracle(s, _lib.RULE_CSHARP, tol, jacobi=jacobi, diag=diag)
    assert ref["status"] == _lib.OK
    assert_equal_runs(solve(s, _lib.RULE_CSHARP, tol, jacobi), ref)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_a_nonzero_initial_guess(dot_order, jacobi):
    s, diag = system("poisson16")
    start = with_b(s, s.b, "poisson16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = sreduce_cg_oracle(start, _lib.RULE_CSHARP, tol, jacobi=jacobi, diag=diag)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, _lib.RULE_CSHARP, tol, jacobi), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, _lib.RULE_SIMPLE, tol, jacobi), reference("poisson16", _lib.RULE_SIMPLE, tol, jacobi))


def test_min_iteration_beyond_convergence(dot_order):
    s, diag = tridiagonal(300)
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = sreduce_cg_oracle(s, _lib.RULE_CSHARP, tol, jacobi=True, diag=diag)
    held = sreduce_cg_oracle(s, _lib.RULE_CSHARP, tol, jacobi=True, diag=diag, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, _lib.RULE_CSHARP, tol, True, min_it=free["iteration"] + 6), held)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_iteration_cap_equals_the_oracle(dot_order, jacobi):
    ref = reference("poisson16", _lib.RULE_CSHARP, 0.0, jacobi, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(system("poisson16")[0], _lib.RULE_CSHARP, 0.0, jacobi, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message("SolveSingleReduce", got, 3)]   # "SolveSingleReduce: did not converge: iteration 4 exceeded maxIteration 3 (residual ...)"


def test_a_trace_shorter_than_the_run(dot_order):
    s, _ = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = dict(reference("poisson16", _lib.RULE_CSHARP, tol, False))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, _lib.RULE_CSHARP, tol, False, trace_capacity=5), ref)


# --------------------------------------------------------------------------- 2. default mode
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_default_dot_order_stays_within_1e_10_of_the_oracle(which, jacobi):
    """Tolerance 1e-13 of || b ||, so that the one iteration the two runs may differ by moves x by far less than the bound: the oracle
    itself moves by at most 2e-14 (2-norm, relative) on these systems when its serial sums are replaced by numpy's pairwise ones."""
    s, _ = system(which)
    tol = 1e-13 * float(np.linalg.norm(s.b))
    ref = reference(which, _lib.RULE_CSHARP, tol, jacobi)
    got = solve(s, _lib.RULE_CSHARP, tol, jacobi)
    distance = float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    print(which, jacobi, "iterations", got["iteration"], ref["iteration"], "distance", distance)
    assert got["status"] == ref["status"] == _lib.OK
    assert abs(got["iteration"] - ref["iteration"]) <= 1
    assert distance <= 1e-10


# --------------------------------------------------------------------------- 3. matrix forms, work space, breakdown
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, jacobi):
    s, _ = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, _lib.RULE_CSHARP, tol, jacobi, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], reference("poisson16", _lib.RULE_CSHARP, tol, jacobi))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, jacobi):
    """NaN in every work vector the caller owns (w, u, r, s).  The direction p lives on the handle's workspace, allocated by the first
    solve: a vector of its size full of NaN is freed just before, which is where the allocator usually takes it from (nothing here can
    check that it did)."""
    s, _ = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR, cg.vectorS):
            v.CopyFrom(nan, s.Count)
        dvec(nan).Dispose()

    assert_equal_runs(solve(s, _lib.RULE_CSHARP, tol, jacobi, prepare=prepare), reference("poisson16", _lib.RULE_CSHARP, tol, jacobi))


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_an_indefinite_matrix_gives_nonfinite_and_the_callers_x_back(dot_order, jacobi):
    ro = np.array([0, 2, 4], dtype=np.int32)
    c = np.array([0, 1, 0, 1], dtype=np.int32)
    s = problems.LinearSystem(np.array([1.0, 2.0, 2.0, 1.0]), c, ro, np.array([0.25, -0.5]), np.array([1.0, -1.0]), "indefinite2")
    ref = sreduce_cg_oracle(s, _lib.RULE_CSHARP, 1e-12, jacobi=jacobi)
    assert ref["status"] == _lib.NONFINITE and np.array_equal(ref["x"], s.x)
    got = solve(s, _lib.RULE_CSHARP, 1e-12, jacobi)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message("SolveSingleReduce", got, NONFINITE)]


def test_a_zero_right_hand_side_gives_nonfinite(dot_order):
    s, diag = tridiagonal(50)
    zero = with_b(s, np.zeros(50), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = sreduce_cg_oracle(zero, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE
        assert_equal_runs(solve(zero, rule, 1e-12, False), ref)


# --------------------------------------------------------------------------- 4. the streaming-hint form of the pass
STREAMING_ROWS = 3_000_001      # the smallest row count at which the pass takes its streaming-hint form (n > 3 000 000); odd: the tail element runs


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_streaming_hint_form_equals_the_oracle(dot_order, jacobi):
    """Six forced bodies, tolerance 0, so that both sides stop at the iteration cap."""
    if "streaming" not in _systems:
        _systems["streaming"] = tridiagonal(STREAMING_ROWS)
    s, diag = _systems["streaming"]
    ref = sreduce_cg_oracle(s, _lib.RULE_CSHARP, 0.0, max_it=5, jacobi=jacobi, diag=diag)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 6
    assert_equal_runs(solve(s, _lib.RULE_CSHARP, 0.0, jacobi, max_it=5), ref)


# --------------------------------------------------------------------------- 5. ranks
def _rank_solve(s, world, rule, tol, jacobi, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, max_it, tol, rank=rank, world=world, comm=comm, rule=rule, device=rank).load(s)
        cg.Initialize()
        if jacobi:
            cg.SetupJacobi()
        cg.SolveSingleReduce(trace=True, jacobi=jacobi)
        cg.Read()
        p = cg.part
        r = np.zeros(max(p.count, 1))
        if p.count:
            cg.vectorR.CopyTo(r, p.count, 0)
        out = dict(offset=p.offset, count=p.count, x=cg.x[p.offset: p.offset + p.count].copy(), r=r[: p.count], iteration=cg.Iteration,
                   residual=cg.Residual, status=cg.status, trace=cg.trace)
        cg.Dispose()
        return out

    return run_ranks(world, make_rank)


def _assert_ranks_equal(res, ref, parts):
    x, r = np.zeros(parts[-1]), np.zeros(parts[-1])
    for k in res:
        x[k["offset"]: k["offset"] + k["count"]] = k["x"]
        r[k["offset"]: k["offset"] + k["count"]] = k["r"]
        assert k["status"] == ref["status"] and k["iteration"] == ref["iteration"] and k["residual"] == ref["residual"]
        assert np.array_equal(k["trace"], ref["trace"])
    assert [k["offset"] for k in res] == parts[:-1]
    assert np.array_equal(x, ref["x"])
    assert np.array_equal(r, ref["r"])


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", ["poisson16", "viennacl4000"])
def test_ranks_equal_the_oracle_with_its_sums_cut_at_their_rows(mgcg_env, dot_order, which, jacobi, world):
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s, _ = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    parts = problems.partition_offsets(s.Count, world)
    ref = reference(which, _lib.RULE_CSHARP, tol, jacobi, parts=parts)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    _assert_ranks_equal(_rank_solve(s, world, _lib.RULE_CSHARP, tol, jacobi), ref, parts)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_a_rank_without_rows_takes_part(mgcg_env, dot_order, jacobi):
    world = 4
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = problems.mgcg_main(3, 160)                      # 3 rows over 4 ranks: offsets [0, 0, 0, 0, 3]
    parts = problems.partition_offsets(s.Count, world)
    assert parts == [0, 0, 0, 0, 3]
    ref = sreduce_cg_oracle(s, _lib.RULE_CSHARP, 1e-8, max_it=50, jacobi=jacobi, parts=parts)
    assert ref["status"] == _lib.OK
    res = _rank_solve(s, world, _lib.RULE_CSHARP, 1e-8, jacobi, max_it=50)
    assert [k["count"] for k in res] == [0, 0, 0, 3]
    _assert_ranks_equal(res, ref, parts)


def test_the_forced_several_ranks_path_on_one_rank_equals_the_one_rank_loop(mgcg_env, dot_order):
    """MGCG_FORCE_MULTIRANK: a one-rank RCCL communicator takes the sums / all-reduce / pass path with a real ncclAllReduce on the stream;
    the sums are the one-rank loop's, so are the bits."""
    import ctypes as C

    L = _lib.lib()
    L.SetDevice(0)
    buf = (C.c_char * 128)()
    assert L.MgcgCommGetUniqueId(buf) == 0, _lib.last_error()
    comm = L.MgcgCommInitRank(buf, 1, 0)
    assert comm, _lib.last_error()
    mgcg_env.setenv("MGCG_FORCE_MULTIRANK", "1")
    s, _ = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    for jacobi in VARIANTS:
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, MAX_IT, tol, rank=0, world=1, comm=comm, rule=_lib.RULE_CSHARP, device=0).load(s)
        cg.Initialize()
        if jacobi:
            cg.SetupJacobi()
        cg.SolveSingleReduce(trace=True, jacobi=jacobi)
        cg.Read()
        r = np.zeros(s.Count)
        cg.vectorR.CopyTo(r, s.Count, 0)
        got = dict(x=cg.x.copy(), r=r, iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace)
        cg.Dispose()
        assert_equal_runs(got, reference("poisson16", _lib.RULE_CSHARP, tol, jacobi))
    L.MgcgCommDestroy(comm)
