"""Multi-shift CG (SolveShifted, shifted.ConjugateGradientShiftedGpu): (A + sigma_j I) x_j = b for k shifts from one CG recurrence on A.

The yardstick is ``shifted_cg_oracle`` below: the loop of include/MgcgGpu.h written with the CPU oracle's primitives -- oracle.spmv,
oracle.dot, oracle.set_added carry the reference's serial arithmetic -- the scalar recurrences in plain Python floats in the contract's
order, and the library's five stop rules (``stop_decision`` of tests/test_gpu_jacobi.py) per column.  Under dot_order = 1 the HIP loop must
EQUAL it; in the default mode only the summation order of the two dots (and of long rows) differs."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.shifted import ConjugateGradientShiftedGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from oracle import oracle as O
from tests.gpu_util import Handles, assert_iterate_close, assert_trace_close, cap_inside_a_chunk, dvec, ivec, same_under_every_chunking
from tests.test_gpu_jacobi import stop_decision

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_HANDMADECL, _lib.RULE_VIENNACL]
MAX_IT = 2000
FINITE_MAX = 1.79e308


# --------------------------------------------------------------------------- the yardstick
def _div(a, b):
    """IEEE division of two Python floats (0 / 0 and x / 0 give NaN and inf instead of raising)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def shifted_scalars(sigma, zeta_k, zeta_prev, alpha_prev, beta_prev, alpha_k, beta_k):
    """zeta_new, alpha_j, beta_j in the contract's order: every product in a float of its own, then the add."""
    t1 = zeta_k * zeta_prev
    num = t1 * alpha_prev
    a1 = alpha_prev * zeta_prev
    s1 = sigma * alpha_k
    s2 = 1.0 + s1
    d1 = a1 * s2
    b1 = alpha_k * beta_prev
    df = zeta_prev - zeta_k
    dd = b1 * df
    den = d1 + dd
    zeta_new = _div(num, den)
    ratio = _div(zeta_new, zeta_k)
    alpha_j = alpha_k * ratio
    q = ratio * ratio
    beta_j = beta_k * q
    return zeta_new, alpha_j, beta_j


def shifted_cg_oracle(s, shifts, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=MAX_IT, dot=None, spmv=None, set_added=None):
    """Returns one dict(x, iteration, residual, status, trace) per shift.  dot / spmv / set_added: the primitives (default: the CPU
    oracle's; tests/test_shifted_host.py plugs numpy's in to test this loop)."""
    dot = dot or O.dot
    spmv = spmv or (lambda v: O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, v))
    set_added = set_added or O.set_added
    k = len(shifts)
    b = np.asarray(s.b, dtype=np.float64)
    r, p = b.copy(), b.copy()
    rr = dot(r, r)
    rr0 = rr
    cols = [dict(x=np.zeros(s.Count), p=b.copy(), zeta=1.0, zeta_prev=1.0, live=True, trace=[], sigma=float(shifts[j])) for j in range(k)]
    alpha_prev, beta_prev, it = 1.0, 0.0, 0
    while any(c["live"] for c in cols):
        Ap = spmv(p)
        pAp = dot(p, Ap)
        alpha = _div(rr, pAp)
        r = set_added(r, Ap, -alpha)
        rr_new = dot(r, r)
        inf = float(np.abs(r).max()) if rule == _lib.RULE_HANDMADECL else 0.0
        beta = _div(rr_new, rr)
        base_broken = not (0.0 < pAp <= FINITE_MAX)
        for c in cols:
            if not c["live"]:
                continue
            zeta_new, alpha_j, beta_j = shifted_scalars(c["sigma"], c["zeta"], c["zeta_prev"], alpha_prev, beta_prev, alpha, beta)
            z2 = zeta_new * zeta_new
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, it, z2 * rr_new, abs(zeta_new) * inf, rr0)
            broken = base_broken or not (abs(zeta_new) <= FINITE_MAX and abs(alpha_j) <= FINITE_MAX and abs(beta_j) <= FINITE_MAX)
            if broken:
                stop, status = True, _lib.NONFINITE
            c["trace"].append(shown)
            if not broken:
                c["x"] = set_added(c["x"], c["p"], alpha_j)
            if stop:
                c.update(live=False, iteration=it, residual=res, status=status)
            else:
                c["p"] = set_added(zeta_new * r, c["p"], beta_j)
                c["zeta_prev"], c["zeta"] = c["zeta"], zeta_new
        p = set_added(r, p, beta)
        rr, alpha_prev, beta_prev = rr_new, alpha, beta
        it += 1
    return [dict(x=c["x"], iteration=c["iteration"], residual=c["residual"], status=c["status"], trace=np.array(c["trace"])) for c in cols]


# --------------------------------------------------------------------------- systems and shifts
def from_zero(s):
    """The same system with the initial guess 0 (what SolveShifted starts every column from)."""
    return problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count), s.b, s.name, s.grid)


def random_spd(n=601):
    """problems.random_spd with another right-hand side (its own b = A 1 is an eigenvector: CG would stop after one step)."""
    s = problems.random_spd(n)
    i = np.arange(n)
    return problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(n), np.cos(0.3 * i) * (1.0 + i % 5), s.name)


SYSTEMS = {
    "ka3_1000": lambda: from_zero(problems.mgcg_main(1000)),            # a row count that is no multiple of 64
    "poisson16": lambda: problems.poisson(16, 16, 16),
    "viennacl4000": lambda: from_zero(problems.viennacl_main(4000)),
    "random_spd601": random_spd,                                         # odd: the columns of x are not all 16-byte aligned (one element at a time)
}
_cache = {}


def system(which):
    if which not in _cache:
        _cache[which] = SYSTEMS[which]()
    return _cache[which]


def diagonal_positions(s):
    """Index of the first stored entry of row i in column i, for every row."""
    ro, c = s.RowOffsets, s.ColumnIndeces
    return np.array([ro[i] + np.nonzero(c[ro[i]: ro[i + 1]] == i)[0][0] for i in range(s.Count)])


def shifted_system(s, sigma):
    """A + sigma I with sigma added to the stored diagonal, the same b, x0 = 0."""
    e = s.Elements[: s.nnz].copy()
    e[diagonal_positions(s)] += sigma
    return problems.LinearSystem(e, s.ColumnIndeces[: s.nnz], s.RowOffsets, np.zeros(s.Count), s.b, s.name, s.grid)


def shifts_for(s, k):
    """Multiples of the mean diagonal d.  k = 8: 0, a repeated value, unsorted, 1e-4 d .. 10 d (five decades); k = 3: 0 and four decades."""
    d = float(np.mean(s.Elements[diagonal_positions(s)]))
    return {1: [1e-2 * d], 3: [10.0 * d, 0.0, 1e-3 * d], 8: [0.1 * d, 0.0, 1e-4 * d, 10.0 * d, 0.1 * d, 1e-3 * d, d, 1e-2 * d]}[k]


def rule_tolerance(s, rule):
    """1e-8 of the first residual's size for the absolute rules (r0 = b), 1e-8 for the relative rule."""
    if rule == _lib.RULE_VIENNACL:
        return 1e-8
    return 1e-8 * (np.abs(s.b).max() if rule == _lib.RULE_HANDMADECL else math.sqrt(O.dot(s.b, s.b)))


_refs = {}


def reference(which, k, rule):
    """The yardstick's run, computed once per case and never changed."""
    key = (which, k, rule)
    if key not in _refs:
        s = system(which)
        _refs[key] = shifted_cg_oracle(s, shifts_for(s, k), rule, rule_tolerance(s, rule))
        for c in _refs[key]:
            c["x"].setflags(write=False)
            c["trace"].setflags(write=False)
    return _refs[key]


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def solve(s, shifts, rule, tol, min_it=0, max_it=MAX_IT, compression=None):
    """One solve through the Python class; an iteration cap that was hit is a result here, not an exception.  One dict per column."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientShiftedGpu(s.Count, maxnz, shifts, min_it, max_it, tol, rule=rule).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    try:
        cg.Solve(trace=True)
    except ApplicationException:
        assert (cg.status == _lib.MAXIT_EXCEEDED).any()
    cg.Read()
    form = _lib.lib().MgcgAnalysisInfo(cg.cusparse, 0, None, None, None, None)      # class of the matrix form the product ran on (-1: plain CSR)
    out = [dict(x=cg.x[j].copy(), iteration=int(cg.Iteration[j]), residual=float(cg.Residual[j]), status=int(cg.status[j]), trace=cg.trace[j], form=form)
           for j in range(len(shifts))]
    cg.Dispose()
    return out


def solve_plain(s, rule, tol, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientSingleGpu(s.Count, maxnz, 0, max_it, tol, rule=rule).load(from_zero(s))
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    out = dict(x=cg.x.copy(), iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace)
    cg.Dispose()
    return out


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"]
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert got["residual"] == ref["residual"]
    assert np.array_equal(got["trace"], ref["trace"])
    assert np.array_equal(got["x"], ref["x"])


def true_residual(s, sigma, x):
    """|| b - (A + sigma I) x || with the oracle's product, in fp64."""
    r = s.b - (O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x) + sigma * x)
    return math.sqrt(O.dot(r, r))


# --------------------------------------------------------------------------- 1. bit equality with the yardstick
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_solve_shifted_equals_the_yardstick_bit_for_bit(oracle, dot_order, which, k, rule):
    s = system(which)
    ref = reference(which, k, rule)
    assert all(c["status"] == _lib.OK and c["iteration"] >= 1 for c in ref)
    got = solve(s, shifts_for(s, k), rule, rule_tolerance(s, rule))
    print(which, k, rule, "iterations", [c["iteration"] for c in got], [c["iteration"] for c in ref])
    if k > 1:
        assert len({c["iteration"] for c in ref}) >= 2          # the columns stop in different iterations: modes 1 and 0 both occur
    for g, c in zip(got, ref):
        assert_equal_runs(g, c)


@pytest.mark.parametrize("which", list(SYSTEMS))
def test_a_column_that_stopped_early_is_left_alone(oracle, dot_order, which):
    """The frozen-column case really occurs (the yardstick's columns stop in at least two different iterations), and the column that stops
    first is, bit for bit, what a k = 1 solve of its shift alone returns: the later iterations of the other columns did not touch it."""
    s = system(which)
    rule, shifts = _lib.RULE_CSHARP, shifts_for(s, 8)
    ref = reference(which, 8, rule)
    stops = [c["iteration"] for c in ref]
    assert len(set(stops)) >= 2, stops
    first = int(np.argmin(stops))
    assert stops[first] < max(stops)
    tol = rule_tolerance(s, rule)
    together = solve(s, shifts, rule, tol)
    alone = solve(s, [shifts[first]], rule, tol)
    print(which, "stops", stops, "column", first)
    assert_equal_runs(together[first], alone[0])
    assert_equal_runs(together[first], ref[first])


# --------------------------------------------------------------------------- 2. the shift 0 is SolveEx
@pytest.mark.parametrize("rule", [_lib.RULE_CSHARP, _lib.RULE_HANDMADECL, _lib.RULE_VIENNACL])
@pytest.mark.parametrize("which", ["poisson16", "random_spd601"])
def test_shift_zero_equals_solve_ex_bit_for_bit(dot_order, which, rule):
    s = system(which)
    tol = rule_tolerance(s, rule)
    plain = solve_plain(s, rule, tol)
    assert plain["status"] == _lib.OK and plain["iteration"] >= 5
    assert_equal_runs(solve(s, [0.0], rule, tol)[0], plain)
    eight = shifts_for(s, 8)
    assert_equal_runs(solve(s, eight, rule, tol)[eight.index(0.0)], plain)


# --------------------------------------------------------------------------- 3. default mode (tree sums)
def yardstick_on_numpy(s, shifts, rule, tol):
    """The yardstick with numpy's dot, product and update: the same loop under another summation order."""
    A = s.to_scipy()
    return shifted_cg_oracle(s, shifts, rule, tol, dot=lambda a, b: float(a @ b), spmv=lambda v: A @ v, set_added=lambda left, right, a: left + a * right)


def stable_floor(trace, other):
    """The lowest of 1e-6, 1e-5, 1e-4 (relative to the first residual) down to which the ORACLE's own trace is stable: the two yardsticks
    agree there to a tenth of assert_trace_close's strict tolerance.  Below it the oracle is chaotic and only the loose bound can be asked."""
    m = min(len(trace), len(other))
    for floor in (1e-6, 1e-5, 1e-4):
        band = trace[:m] >= floor * trace[0]
        if np.all(np.abs(trace[:m][band] - other[:m][band]) <= 1e-11 * trace[:m][band]):
            return floor
    raise AssertionError("the yardstick itself is not stable down to 1e-4 of the first residual")


@pytest.mark.parametrize("which", list(SYSTEMS))
def test_default_mode_within_the_north_star(oracle, which):
    """The relative rule at 1e-6 (tests/test_gpu_jacobi.py's choice): every column stops where assert_trace_close's strict band ends.  The
    strict band of a column is cut short only where the oracle itself moves under another summation order (stable_floor: computed, and on
    three of the four systems 1e-6; random_spd601's plain CG -- the shift-0 column, bit for bit -- moves by 3e-5 below 1e-5), and the iterate
    gets assert_iterate_close's spread argument from the same second yardstick."""
    s = system(which)
    shifts = shifts_for(s, 8)
    ref = shifted_cg_oracle(s, shifts, _lib.RULE_VIENNACL, 1e-6)
    other = yardstick_on_numpy(s, shifts, _lib.RULE_VIENNACL, 1e-6)
    got = solve(s, shifts, _lib.RULE_VIENNACL, 1e-6)
    for j, (g, c, o) in enumerate(zip(got, ref, other)):
        assert g["status"] == c["status"] == _lib.OK
        assert g["iteration"] == c["iteration"], (j, g["iteration"], c["iteration"])
        floor = stable_floor(c["trace"], o["trace"])
        assert_trace_close(g["trace"], c["trace"], floor=floor)
        print(which, j, "iterations", g["iteration"], "strict down to", floor, "distance, spread", assert_iterate_close(g["x"], c["x"], spread_refs=[o["x"]]))


# --------------------------------------------------------------------------- 4. the true residual
TRUE_RESIDUAL_FACTOR = 1.001


@pytest.mark.parametrize("which", list(SYSTEMS))
def test_true_residual_against_plain_cg_on_the_shifted_matrix(oracle, which):
    """|| b - (A + sigma_j I) x_j || of every column against the true residual that oracle.cg leaves on the explicitly shifted matrix at the
    same tolerance (RULE_CSHARP, 1e-8 of || b ||).  The recurrence's residual zeta_j r drifts from the true one as any CG's does; how far was
    measured once with the YARDSTICK (not the HIP loop) on these four systems and eight shifts each: yardstick / oracle.cg between 0.978 and
    1.00027 (both on random_spd601; within 2.1e-7 of 1 on the other three), so the allowed factor is 1.001, asserted with a margin of 2 for the drift."""
    s = system(which)
    shifts = shifts_for(s, 8)
    tol = rule_tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, shifts, _lib.RULE_CSHARP, tol)
    for j, sigma in enumerate(shifts):
        plain = O.cg(shifted_system(s, sigma), rule=O.RULE_CSHARP, allowable_residual=tol, max_iteration=MAX_IT)
        assert plain["status"] == _lib.OK and got[j]["status"] == _lib.OK
        mine, theirs = true_residual(s, sigma, got[j]["x"]), true_residual(s, sigma, plain["x"])
        print(which, j, "sigma", sigma, "true residual", mine, "plain CG on the shifted matrix", theirs, "ratio", mine / theirs)
        assert mine <= 2.0 * TRUE_RESIDUAL_FACTOR * theirs


# --------------------------------------------------------------------------- 5. compression modes, streaming-hint form
def test_compressed_forms_give_the_same_bits(dot_order):
    """Under dot_order = 1: every form's product is bit-identical, but in the default mode the best form groups the fused p.Ap partial sums
    by other row blocks than plain CSR does (tests/test_gpu_dcsr.py says so for SolveEx), which moves the last bits of every scalar."""
    s = system("poisson16")
    shifts = shifts_for(s, 3)
    runs = [solve(s, shifts, _lib.RULE_CSHARP, 1e-8, compression=mode) for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES)]
    assert all(c["status"] == _lib.OK and c["iteration"] >= 3 for c in runs[0])
    assert runs[0][0]["form"] == -1 and runs[1][0]["form"] >= 1 and runs[2][0]["form"] >= 1, [r[0]["form"] for r in runs]      # compressed forms were really used
    for other in runs[1:]:
        for g, c in zip(other, runs[0]):
            assert_equal_runs(g, c)


STREAMING_ROWS = 3_000_002      # just above the size from which the vector passes take their streaming-hint forms (n > 3 000 000); even: 16-byte accesses


def test_streaming_hint_form_equals_the_yardstick_bit_for_bit(oracle, dot_order):
    """The fused pass above 3 M rows (non-temporal loads and stores): five forced iterations on a tridiagonal system, tolerance 0, so that
    every column stops at the iteration cap."""
    from tests.test_gpu_jacobi import tridiagonal

    s, _ = tridiagonal(STREAMING_ROWS)
    shifts = [3.0, 0.0]
    ref = shifted_cg_oracle(s, shifts, _lib.RULE_CSHARP, 0.0, max_it=4)
    assert all(c["status"] == _lib.MAXIT_EXCEEDED and c["iteration"] == 5 for c in ref)
    got = solve(s, shifts, _lib.RULE_CSHARP, 0.0, max_it=4)
    for g, c in zip(got, ref):
        assert_equal_runs(g, c)


# --------------------------------------------------------------------------- 6. errors
def _raw_call(h, vecs, s, k, shifts, x=None, max_it=50, tol=1e-8):
    """SolveShifted through the C ABI; returns (status, per-column status)."""
    L = _lib.lib()
    status = np.full(8, -7, dtype=np.int32)
    sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64)
    L.MgcgClearLastError()
    st = L.SolveShifted(h.blas, h.sparse, h.descr, vecs["e"].Ptr, vecs["r"].Ptr, vecs["c"].Ptr, (x or vecs["x"]).Ptr, vecs["b"].Ptr,
                        vecs["Ap"].Ptr, vecs["p"].Ptr, vecs["res"].Ptr, vecs["ps"].Ptr, s.nnz, s.Count, k,
                        None if sh is None else sh.ctypes.data_as(C.c_void_p), tol, 0, max_it, _lib.RULE_CSHARP,
                        None, None, status.ctypes.data_as(C.c_void_p), None, 0)
    return st, status


def _vectors(s, k=8):
    n = s.Count
    return dict(e=dvec(s.Elements[: s.nnz]), c=ivec(s.ColumnIndeces[: s.nnz]), r=ivec(s.RowOffsets), x=dvec(np.full(k * n, 7.0)), b=dvec(s.b),
                Ap=dvec(np.zeros(n)), p=dvec(np.zeros(n)), res=dvec(np.zeros(n)), ps=dvec(np.zeros(k * n)))


def test_bad_arguments_are_refused_with_a_message_and_nothing_runs():
    s = problems.poisson(8, 8, 8)
    h, v = Handles(), _vectors(s)
    cases = [(0, [1.0], None, "k = 0"), (9, [1.0] * 9, None, "k = 9"), (2, [1.0, -0.5], None, "shift 1"), (2, [float("nan"), 1.0], None, "shift 0"),
             (2, [float("inf"), 1.0], None, "shift 0"), (2, None, None, "NULL"), (3, [0.0, 1.0, 2.0], dvec(np.zeros(3 * s.Count - 1)), "smaller")]
    for k, shifts, x, word in cases:
        st, _ = _raw_call(h, v, s, k, shifts, x=x)
        msg = _lib.last_error()
        _lib.lib().MgcgClearLastError()
        print(k, shifts, msg)
        assert st == _lib.ERROR and word in msg, (k, shifts, msg)
        assert np.array_equal(v["x"].to_numpy(8 * s.Count), np.full(8 * s.Count, 7.0))          # x was not touched: nothing was enqueued
    full = v["ps"]
    v["ps"] = dvec(np.zeros(3 * s.Count - 1))                  # a direction work space that is too small
    st, _ = _raw_call(h, v, s, 3, [0.0, 1.0, 2.0])
    assert st == _lib.ERROR and "smaller" in _lib.last_error()
    v["ps"] = full
    _lib.lib().MgcgClearLastError()
    assert np.array_equal(v["x"].to_numpy(8 * s.Count), np.full(8 * s.Count, 7.0))
    h.close()


def test_an_indefinite_matrix_ends_with_nonfinite_and_returns():
    s = problems.poisson(8, 8, 8)
    e = -s.Elements[: s.nnz]                                   # negative definite: p.Ap < 0 in the first iteration
    neg = problems.LinearSystem(e, s.ColumnIndeces[: s.nnz], s.RowOffsets, np.zeros(s.Count), s.b, "negative")
    h, v = Handles(), _vectors(neg, 2)
    st, status = _raw_call(h, v, neg, 2, [0.0, 1.0])
    assert st == _lib.NONFINITE and list(status[:2]) == [_lib.NONFINITE] * 2 and "broke down" in _lib.last_error()
    _lib.lib().MgcgClearLastError()
    assert np.array_equal(v["x"].to_numpy(2 * s.Count), np.zeros(2 * s.Count))     # the last good iterate: the start
    _lib.lib().MgcgClearLastError()
    h.close()
    cg = ConjugateGradientShiftedGpu(s.Count, 7, [0.0, 1.0], 0, 50, 1e-8, rule=_lib.RULE_CSHARP).load(neg)
    cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="broke down"):
        cg.Solve()
    cg.Dispose()


def test_iteration_cap_is_reported_per_column_and_raises_in_python():
    s = system("poisson16")
    d = float(np.mean(s.Elements[diagonal_positions(s)]))
    shifts = [100.0 * d, 0.0]                                  # the first converges in a few iterations, the second cannot within 5
    cg = ConjugateGradientShiftedGpu(s.Count, 7, shifts, 0, 5, 1e-10, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    with pytest.raises(ApplicationException):
        cg.Solve()
    assert list(cg.status) == [_lib.OK, _lib.MAXIT_EXCEEDED] and cg.Iteration[0] <= 5 and cg.Iteration[1] == 6
    assert not _lib.last_error()
    cg.Dispose()


# --------------------------------------------------------------------------- 7. the class, from load() to Read()
def test_python_class_round_trip():
    s = system("poisson16")
    shifts = shifts_for(s, 3)
    cg = ConjugateGradientShiftedGpu(s.Count, 7, shifts, 0, MAX_IT, 1e-9, rule=_lib.RULE_CSHARP).load(s)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    assert cg.x.shape == (3, s.Count) and cg.Iteration.shape == cg.Residual.shape == cg.status.shape == (3,)
    assert (cg.status == _lib.OK).all() and (cg.Residual < 1e-9).all() and len(cg.trace) == 3
    for j, sigma in enumerate(shifts):
        assert len(cg.trace[j]) == cg.Iteration[j] + 1 and cg.trace[j][-1] == cg.Residual[j]
        assert true_residual(s, sigma, cg.x[j]) < 1e-8
    cg.Initialize()                                            # a second solve on the same object gives the same bits
    first = cg.x.copy()
    cg.Solve()
    cg.Read()
    assert np.array_equal(cg.x, first)
    cg.Dispose()


# --------------------------------------------------------------------------- 8. the host's chunking
@pytest.mark.parametrize("order", [0, 1])
def test_chunking_cannot_change_a_result(order):
    """check_every = 1, 4, 7 on 8^3 Poisson with 3 shifts: the same bits, also when the iteration cap ends columns in the middle of a chunk."""
    s = problems.poisson(8, 8, 8)
    shifts = shifts_for(s, 3)

    def run(max_it):
        cols = solve(s, shifts, _lib.RULE_VIENNACL, 1e-8, max_it=max_it)
        return {key: [c[key] for c in cols] for key in ("x", "iteration", "residual", "status", "trace")}

    free = same_under_every_chunking(lambda: run(MAX_IT), order)
    its = free["iteration"]
    print("iterations", its)
    assert free["status"] == [_lib.OK] * 3 and len(set(its)) > 1, (free["status"], its)
    cap = cap_inside_a_chunk(min(its), max(its))
    capped = same_under_every_chunking(lambda: run(cap), order)
    print("cap", cap, "status", capped["status"])
    assert _lib.MAXIT_EXCEEDED in capped["status"] and max(capped["iteration"]) == cap + 1
