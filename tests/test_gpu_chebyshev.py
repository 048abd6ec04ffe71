"""Chebyshev-preconditioned CG on the GPU (MgcgGershgorinBound, SolveChebyshev, SolveChebyshevParallel,
chebyshev.ConjugateGradientChebyshevGpu, ConjugateGradientRankGpu.SolveChebyshev).

The reference for every comparison is ``chebyshev_cg_oracle`` (tests/test_chebyshev_host.py): the header's loop in numpy with serial sums.
Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and trace, iteration, residual, status and ALL of x and r must
EQUAL it; in the default mode only the summation order of the sums (and of long rows) differs."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.chebyshev import ConjugateGradientChebyshevGpu, gershgorin_bound
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from tests.gpu_util import ivec, library_messages, maxit_message, nonfinite_message
from tests.test_chebyshev_host import chebyshev_cg_oracle, default_bounds, gershgorin_oracle
from tests.test_gpu_jacobi import run_ranks
from tests.test_sreduce_host import diagonal_of, randn_b, tridiagonal, with_b

pytestmark = pytest.mark.gpu

VARIANTS = [False, True]
DEGREES = [1, 2, 3, 8]               # odd and even degrees end in different z buffers
MAX_IT = 3000
# what MGCG_NONFINITE means in this loop, as the library words it (csrc/solver.hip: cg_solve_chebyshev)
NONFINITE = "p.Ap or r.z is not finite and > 0 (an upper bound below the spectrum makes the polynomial indefinite), or the residual is not finite"

SYSTEMS = {
    "tridiagonal300": lambda: tridiagonal(300)[0],
    "poisson16": lambda: randn_b(problems.poisson(16, 16, 16), "poisson16"),
    "viennacl4000": lambda: problems.viennacl_main(4000, 40),
}
_systems, _oracles = {}, {}


def system(name):
    """(system, diagonal, {jacobi: the default bounds: Gershgorin / 30})."""
    if name not in _systems:
        s = SYSTEMS[name]()
        diag = diagonal_of(s)
        _systems[name] = (s, diag, {False: default_bounds(s), True: default_bounds(s, 1.0 / diag)})
    return _systems[name]


def reference(name, degree, rule, tol, jacobi, parts=None, bounds=None, **kw):
    """The oracle's run, computed once per case and shared (nothing changes it)."""
    key = (name, degree, rule, tol, jacobi, None if parts is None else tuple(parts), bounds, tuple(sorted(kw.items())))
    if key not in _oracles:
        s, diag, b = system(name)
        _oracles[key] = chebyshev_cg_oracle(s, degree, b[jacobi] if bounds is None else bounds, rule, tol, jacobi=jacobi, diag=diag, parts=parts,
                                            **{"max_it": MAX_IT, **kw})
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


def solve(s, degree, bounds, rule, tol, jacobi, min_it=0, max_it=MAX_IT, compression=None, kernel=None, trace_capacity=None, prepare=None):
    """One solve through the Python class; an iteration cap that was hit is a result here, not an exception.  prepare(cg): after Initialize()."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientChebyshevGpu(s.Count, maxnz, min_it, max_it, tol, rule=rule, degree=degree, jacobi=jacobi, bounds=bounds).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    if kernel is not None:
        _lib.lib().MgcgSetSpmvKernel(cg.cusparse, kernel)
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
    out = dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace,
               bounds=(cg.lambdaMin, cg.lambdaMax), messages=list(said))
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
def _equals_the_oracle(which, degree, jacobi, rule):
    s, _, bounds = system(which)
    tol = tolerance(s, rule)
    ref = reference(which, degree, rule, tol, jacobi)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, degree, bounds[jacobi], rule, tol, jacobi)
    print(which, degree, jacobi, rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, jacobi, degree):
    _equals_the_oracle(which, degree, jacobi, _lib.RULE_CSHARP)


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_the_other_rules_equal_the_oracle_bit_for_bit(dot_order, which, jacobi, degree, rule):
    _equals_the_oracle(which, degree, jacobi, rule)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("n", [1, 7, 300, 257 * 3])
def test_small_and_odd_sizes_equal_the_oracle(dot_order, n, jacobi):
    """Less than a workgroup, no multiple of 256 or of the 16-byte access, more than one tile of the row-tile kernel."""
    s, diag = tridiagonal(n)
    tol = 1e-10 * float(np.linalg.norm(s.b))
    bounds = default_bounds(s, 1.0 / diag if jacobi else None)
    ref = chebyshev_cg_oracle(s, 3, bounds, _lib.RULE_CSHARP, tol, jacobi=jacobi, diag=diag)
    assert ref["status"] == _lib.OK
    assert_equal_runs(solve(s, 3, bounds, _lib.RULE_CSHARP, tol, jacobi), ref)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("kernel", [10, 9, 1])
def test_each_plain_csr_kernel_runs_both_epilogues_and_gives_the_same_bits(dot_order, kernel, jacobi):
    """The row-tile, the row-block and the stream form, forced: degree 3 runs EPI_CHEBYSHEV and EPI_CHEBYSHEV_DOT in every iteration."""
    for which in ("poisson16", "tridiagonal300"):
        s, _, bounds = system(which)
        tol = tolerance(s, _lib.RULE_CSHARP)
        assert_equal_runs(solve(s, 3, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi, kernel=kernel), reference(which, 3, _lib.RULE_CSHARP, tol, jacobi))


def test_the_lanes_per_row_kernel_runs_both_epilogues():
    """kernels_spmv.hip's second kernel adds a row lane by lane, not in stored order: the same method within round-off."""
    s, _, bounds = system("viennacl4000")
    tol = 1e-13 * float(np.linalg.norm(s.b))
    ref = reference("viennacl4000", 3, _lib.RULE_CSHARP, tol, True)
    got = solve(s, 3, bounds[True], _lib.RULE_CSHARP, tol, True, kernel=6)
    assert got["status"] == ref["status"] == _lib.OK and abs(got["iteration"] - ref["iteration"]) <= 1
    assert float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"])) <= 1e-10


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, jacobi):
    s, _, bounds = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, 3, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], reference("poisson16", 3, _lib.RULE_CSHARP, tol, jacobi))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


# --------------------------------------------------------------------------- 2. the Jacobi anchor
@pytest.mark.parametrize("serial", [True, False], ids=["dot_order", "default"])
@pytest.mark.parametrize("which", ["tridiagonal300", "viennacl4000"])
def test_degree_one_with_theta_one_equals_the_jacobi_loop_exactly(mgcg_env, which, serial):
    """it = 1 / 1.0: d = 1 * (dinv r) is dinv r bit for bit, and the passes walk their elements as the Jacobi loop's do: the same x, trace and
    iteration whatever the order of the sums."""
    if serial:
        mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    s, _, _ = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientJacobiGpu(s.Count, maxnz, 0, MAX_IT, tol, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    want = dict(x=cg.x.copy(), iteration=cg.Iteration, residual=cg.Residual, trace=cg.trace)
    cg.Dispose()
    got = solve(s, 1, (0.5, 1.5), _lib.RULE_CSHARP, tol, True)
    assert got["status"] == _lib.OK and want["iteration"] >= 3
    assert got["iteration"] == want["iteration"] and got["residual"] == want["residual"]
    assert np.array_equal(got["trace"], want["trace"]) and np.array_equal(got["x"], want["x"])


# --------------------------------------------------------------------------- 3. the loop's other behaviour
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_a_nonzero_initial_guess(dot_order, jacobi):
    s, diag, bounds = system("poisson16")
    start = with_b(s, s.b, "poisson16-x0")
    start.x[:] = 0.5 * np.cos(0.01 * np.arange(s.Count))
    tol = 1e-8 * float(np.linalg.norm(s.b))
    ref = chebyshev_cg_oracle(start, 2, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi=jacobi, diag=diag)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert_equal_runs(solve(start, 2, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi), ref)
    # ... which MGCG_RULE_SIMPLE ignores
    assert_equal_runs(solve(start, 2, bounds[jacobi], _lib.RULE_SIMPLE, tol, jacobi), reference("poisson16", 2, _lib.RULE_SIMPLE, tol, jacobi))


def test_min_iteration_beyond_convergence(dot_order):
    s, diag, bounds = system("tridiagonal300")
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = chebyshev_cg_oracle(s, 2, bounds[True], _lib.RULE_CSHARP, tol, jacobi=True, diag=diag)
    held = chebyshev_cg_oracle(s, 2, bounds[True], _lib.RULE_CSHARP, tol, jacobi=True, diag=diag, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, 2, bounds[True], _lib.RULE_CSHARP, tol, True, min_it=free["iteration"] + 6), held)


@pytest.mark.parametrize("degree", [1, 4])
def test_iteration_cap_equals_the_oracle(dot_order, degree):
    ref = reference("poisson16", degree, _lib.RULE_CSHARP, 0.0, False, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    s, _, bounds = system("poisson16")
    got = solve(s, degree, bounds[False], _lib.RULE_CSHARP, 0.0, False, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message("SolveChebyshev", got, 3)]      # "SolveChebyshev: did not converge: iteration 4 exceeded maxIteration 3 (residual ...)"


def test_a_trace_shorter_than_the_run(dot_order):
    s, _, bounds = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = dict(reference("poisson16", 2, _lib.RULE_CSHARP, tol, False))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, 2, bounds[False], _lib.RULE_CSHARP, tol, False, trace_capacity=5), ref)


@pytest.mark.parametrize("degree", [2, 3])
def test_garbage_in_the_work_space_does_not_reach_the_result(dot_order, degree):
    """NaN in every work vector the caller owns (Ap, p, r, z, z2, d)."""
    s, _, bounds = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    nan = np.full(s.Count, np.nan)

    def prepare(cg):
        for v in (cg.vectorAp, cg.vectorP, cg.vectorR, cg.vectorZ, cg.vectorZ2, cg.vectorD):
            v.CopyFrom(nan, s.Count)

    assert_equal_runs(solve(s, degree, bounds[True], _lib.RULE_CSHARP, tol, True, prepare=prepare), reference("poisson16", degree, _lib.RULE_CSHARP, tol, True))


# --------------------------------------------------------------------------- 4. breakdown
def test_an_upper_bound_below_the_spectrum_gives_nonfinite_and_the_callers_x_back(dot_order):
    s, _, bounds = system("tridiagonal300")
    start = with_b(s, s.b, "tridiagonal300-x0")
    start.x[:] = 1e-3 * np.sin(np.arange(300))
    lmax = bounds[False][1] / 4.0
    for which in (s, start):
        ref = chebyshev_cg_oracle(which, 2, (lmax / 30.0, lmax), _lib.RULE_CSHARP, 1e-8)
        assert ref["first_rz"] < 0.0 and ref["status"] == _lib.NONFINITE and ref["iteration"] == 0 and np.array_equal(ref["x"], which.x)
        got = solve(which, 2, (lmax / 30.0, lmax), _lib.RULE_CSHARP, 1e-8, False)
        assert_equal_runs(got, ref)
        assert got["messages"] == [nonfinite_message("SolveChebyshev", got, NONFINITE)]


def test_a_zero_right_hand_side_gives_nonfinite(dot_order):
    s, _, bounds = system("tridiagonal300")
    zero = with_b(s, np.zeros(300), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = chebyshev_cg_oracle(zero, 3, bounds[False], rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE
        assert_equal_runs(solve(zero, 3, bounds[False], rule, 1e-12, False), ref)


# --------------------------------------------------------------------------- 5. default mode
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_default_dot_order_stays_within_1e_10_of_the_oracle(which, jacobi):
    """Tolerance 1e-13 of || b ||, so that the one iteration the two runs may differ by moves x by far less than the bound."""
    s, _, bounds = system(which)
    tol = 1e-13 * float(np.linalg.norm(s.b))
    ref = reference(which, 4, _lib.RULE_CSHARP, tol, jacobi)
    got = solve(s, 4, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi)
    distance = float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    print(which, jacobi, "iterations", got["iteration"], ref["iteration"], "distance", distance)
    assert got["status"] == ref["status"] == _lib.OK
    assert abs(got["iteration"] - ref["iteration"]) <= 1
    assert distance <= 1e-10


# --------------------------------------------------------------------------- 6. the bound and the class default
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_the_gershgorin_bound_equals_its_oracle(which):
    s, diag, _ = system(which)
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientJacobiGpu(s.Count, maxnz, 0, 10, 1e-8).load(s)
    cg.Initialize()
    args = (cg.cusparse, cg.vectorA, cg.vectorRowOffsets, cg.vectorColumnIndeces, s.nnz, s.Count, 0)
    assert gershgorin_bound(*args) == gershgorin_oracle(s)
    assert gershgorin_bound(*args, cg.vectorDinv) == gershgorin_oracle(s, 1.0 / diag)
    # a slice of the rows, as a rank would ask
    lo, hi = s.Count // 3, min(s.Count // 3 + 257, s.Count)
    ro = np.asarray(s.RowOffsets[lo: hi + 1])
    vro = ivec(ro)
    bound = C.c_double(0.0)
    assert _lib.lib().MgcgGershgorinBound(cg.cusparse, cg.vectorA.Ptr, vro.Ptr, cg.vectorColumnIndeces.Ptr, s.nnz, hi - lo, lo, None, C.byref(bound)) == 0
    assert bound.value == gershgorin_oracle(s, None, lo, hi)
    vro.Dispose()
    cg.Dispose()


def test_the_class_default_bounds_solve_in_fewer_iterations_than_plain_cg():
    s, _, bounds = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, 4, None, _lib.RULE_CSHARP, tol, False)
    assert got["bounds"] == (12.0 / 30.0, 12.0) == bounds[False]
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientSingleGpu(s.Count, maxnz, 0, MAX_IT, tol, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    cg.Solve()
    plain = cg.Iteration
    cg.Dispose()
    print("16^3 Poisson: degree 4", got["iteration"], "iterations, plain CG", plain)
    assert got["status"] == _lib.OK and got["iteration"] < plain
    x = got["x"]
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    r = s.b - np.bincount(rows, weights=s.Elements[: s.nnz] * x[s.ColumnIndeces[: s.nnz]], minlength=s.Count)
    assert np.linalg.norm(r) < 1.01 * tol


# --------------------------------------------------------------------------- 7. ranks
def _rank_solve(s, world, degree, bounds, rule, tol, jacobi, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, max_it, tol, rank=rank, world=world, comm=comm, rule=rule, device=rank).load(s)
        cg.Initialize()
        if jacobi:
            cg.SetupJacobi()
        cg.SolveChebyshev(trace=True, jacobi=jacobi, degree=degree, bounds=bounds)
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
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
@pytest.mark.parametrize("which", ["poisson16", "viennacl4000"])
def test_ranks_equal_the_oracle_with_its_sums_cut_at_their_rows(mgcg_env, dot_order, which, jacobi, degree, world):
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s, _, bounds = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    parts = problems.partition_offsets(s.Count, world)
    ref = reference(which, degree, _lib.RULE_CSHARP, tol, jacobi, parts=parts)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    _assert_ranks_equal(_rank_solve(s, world, degree, bounds[jacobi], _lib.RULE_CSHARP, tol, jacobi), ref, parts)


@pytest.mark.parametrize("jacobi", VARIANTS, ids=["plain", "jacobi"])
def test_a_rank_without_rows_takes_part(mgcg_env, dot_order, jacobi):
    world = 4
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = problems.mgcg_main(3, 160)                      # 3 rows over 4 ranks: offsets [0, 0, 0, 0, 3]
    parts = problems.partition_offsets(s.Count, world)
    assert parts == [0, 0, 0, 0, 3]
    diag = diagonal_of(s)
    bounds = default_bounds(s, 1.0 / diag if jacobi else None)
    ref = chebyshev_cg_oracle(s, 2, bounds, _lib.RULE_CSHARP, 1e-8, max_it=50, jacobi=jacobi, parts=parts, diag=diag)
    assert ref["status"] == _lib.OK
    res = _rank_solve(s, world, 2, bounds, _lib.RULE_CSHARP, 1e-8, jacobi, max_it=50)
    assert [k["count"] for k in res] == [0, 0, 0, 3]
    _assert_ranks_equal(res, ref, parts)


def test_the_forced_several_ranks_path_on_one_rank_equals_the_one_rank_loop(mgcg_env, dot_order):
    """MGCG_FORCE_MULTIRANK: a one-rank RCCL communicator takes the reduce / all-reduce path with a real ncclAllReduce on the stream; the
    sums are the one-rank loop's, so are the bits."""
    L = _lib.lib()
    L.SetDevice(0)
    buf = (C.c_char * 128)()
    assert L.MgcgCommGetUniqueId(buf) == 0, _lib.last_error()
    comm = L.MgcgCommInitRank(buf, 1, 0)
    assert comm, _lib.last_error()
    mgcg_env.setenv("MGCG_FORCE_MULTIRANK", "1")
    s, _, bounds = system("poisson16")
    tol = tolerance(s, _lib.RULE_CSHARP)
    maxnz = int(np.diff(s.RowOffsets).max())
    for jacobi, degree in ((False, 3), (True, 2), (True, 1)):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, MAX_IT, tol, rank=0, world=1, comm=comm, rule=_lib.RULE_CSHARP, device=0).load(s)
        cg.Initialize()
        if jacobi:
            cg.SetupJacobi()
        cg.SolveChebyshev(trace=True, jacobi=jacobi, degree=degree, bounds=bounds[jacobi])
        cg.Read()
        r = np.zeros(s.Count)
        cg.vectorR.CopyTo(r, s.Count, 0)
        got = dict(x=cg.x.copy(), r=r, iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace)
        cg.Dispose()
        assert_equal_runs(got, reference("poisson16", degree, _lib.RULE_CSHARP, tol, jacobi))
    L.MgcgCommDestroy(comm)
