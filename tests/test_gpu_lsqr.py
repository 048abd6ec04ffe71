"""LSQR on the GPU (MgcgSolveLsqr, lsqr.LeastSquaresGpu).

The reference for every comparison is ``lsqr_oracle`` (tests/test_lsqr_host.py): the header's loop in numpy with serial sums and the A^T
of ``transpose_arrays``.  Under dot_order = 1 the HIP loop is a fixed sequence of IEEE operations and status, iteration, residual, the
residual norm's estimate, both true figures, the trace and ALL of x and of the two closing vectors must EQUAL it; in the default mode
only the summation order of the sums (and of long rows) differs."""
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.lsqr import LeastSquaresGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import library_messages, maxit_message, nonfinite_message
from tests.test_lsqr_host import CASES, NOT_EXHAUSTED, SEED, g0_of, lsqr_oracle, orthogonal_rhs, system
from tests.test_transpose_host import transpose_arrays

pytestmark = pytest.mark.gpu

MAX_IT = 2000
REL = 1e-10
_oracles = {}
# what MGCG_NONFINITE means at the start, as the library words it (csrc/solver.hip: lsqr_solve)
NONFINITE_BETA = "beta_1 = || b || is zero or not finite"
NONFINITE_ALPHA = "alpha_1 = || A^T b || / beta_1 is zero or not finite (a nonzero b is orthogonal to the range of A)"


def reference(name, damp, rule, tol, **kw):
    """The oracle's run, computed once per case and shared (nothing changes it)."""
    key = (name, damp, rule, tol, tuple(sorted(kw.items())))
    if key not in _oracles:
        _oracles[key] = lsqr_oracle(system(name), damp, rule, tol, **{"max_it": MAX_IT, **kw})
        for v in _oracles[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _oracles[key]


def tolerance(s, rule, rel=REL):
    """The relative rule: rel; the absolute rules: rel of g0 = || A^T b ||."""
    return rel if rule == _lib.RULE_VIENNACL else rel * g0_of(s)


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def solve(s, damp, rule, tol, min_it=0, max_it=MAX_IT, compression=None, trace_capacity=None, prepare=None, inspect=None):
    """One solve through the Python class; an iteration cap that was hit or a breakdown is a result here, not an exception.
    prepare(cg): after Initialize(); inspect(cg): after the solve."""
    maxnz = max(int(np.diff(s.RowOffsets).max()), 1)
    cg = LeastSquaresGpu(s.Rows, s.Columns, maxnz, min_it, max_it, tol, rule=rule, damp=damp).load(s)
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
    out = dict(x=cg.x.copy(), r=cg.ReadResidual(), t=cg.ReadNormalResidual(), iteration=cg.Iteration, residual=cg.Residual,
               residual_norm=cg.ResidualNorm, true_residual=cg.TrueResidual, true_normal_residual=cg.TrueNormalResidual,
               status=cg.status, trace=cg.trace, messages=list(said))
    if inspect is not None:
        inspect(cg)
    cg.Dispose()
    return out


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    for key in ("residual", "residual_norm", "true_residual", "true_normal_residual"):
        assert same(got[key], ref[key]), (key, got[key], ref[key])
    assert np.array_equal(got["trace"], ref["trace"], equal_nan=True)
    for key in ("x", "r", "t"):
        assert np.array_equal(got[key], ref[key], equal_nan=True), key


# --------------------------------------------------------------------------- 1. bit equality with the oracle
DAMPED = ("rect771x257", "rect257x771", "banded700x1900", "convdiff12x10x8")
RULE_CASES = ([(n, 0.0, _lib.RULE_CSHARP) for n in CASES] + [(n, 0.5, _lib.RULE_CSHARP) for n in DAMPED] +
              [("rect771x257", 0.5, _lib.RULE_NATIVE), ("banded1900x700", 0.0, _lib.RULE_SIMPLE), ("rect257x771", 0.5, _lib.RULE_VIENNACL)])


@pytest.mark.parametrize("which,damp,rule", RULE_CASES)
def test_solve_equals_the_oracle_bit_for_bit(dot_order, which, damp, rule):
    s = system(which)
    tol = tolerance(s, rule)
    ref = reference(which, damp, rule, tol)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3, ref["iteration"]
    got = solve(s, damp, rule, tol)
    print(which, damp, rule, "bodies", got["iteration"], ref["iteration"], "g", got["residual"], ref["residual"],
          "true normal", got["true_normal_residual"], ref["true_normal_residual"])
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 2. shapes
def band(rows, columns, name=None):
    """A bidiagonal-like rectangular band: row i stores columns i mod columns and (with more than one column) (i + 1) mod columns, in that
    order; b = N(0,1)."""
    i = np.arange(rows)
    per = 2 if columns > 1 else 1
    c = np.stack([i % columns, (i + 1) % columns], axis=1)[:, :per]
    e = np.stack([2.0 + i % 3, -1.0 - 0.5 * (i % 2)], axis=1)[:, :per]
    ro = (np.arange(rows + 1) * per).astype(np.int32)
    return problems.LeastSquaresSystem(np.ascontiguousarray(e.reshape(-1), dtype=np.float64), np.ascontiguousarray(c.reshape(-1), dtype=np.int32), ro,
                                       np.random.default_rng(SEED).standard_normal(rows), columns, name or f"band{rows}x{columns}")


@pytest.mark.parametrize("damp", [0.0, 0.25])
@pytest.mark.parametrize("rows,columns", [(1, 1), (1, 5), (5, 1), (2, 3), (7, 300), (300, 7), (257, 771), (771, 257)])
def test_small_and_odd_shapes_equal_the_oracle(dot_order, rows, columns, damp):
    """Fewer lanes than a workgroup, counts that are no multiple of 256 nor of two (the 16-byte tail), more than one workgroup in one
    dimension and not in the other; the smallest end by g == 0 or at rounding level."""
    s = band(rows, columns)
    tol = REL * g0_of(s)
    ref = lsqr_oracle(s, damp, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    assert ref["status"] == _lib.OK
    assert_equal_runs(solve(s, damp, _lib.RULE_CSHARP, tol), ref)


STREAMING = (3_000_001, 3_000_003)     # both counts beyond 3 000 000, where the passes take their streaming-hint form; odd: the tail element runs
_streaming = {}


def test_streaming_hint_form_equals_the_oracle(dot_order):
    """Four forced bodies, tolerance 0, so that both sides stop at the iteration cap."""
    if "s" not in _streaming:
        _streaming["s"] = band(*STREAMING)
    s = _streaming["s"]
    ref = lsqr_oracle(s, 0.5, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    assert_equal_runs(solve(s, 0.5, _lib.RULE_CSHARP, 0.0, max_it=3), ref)


# --------------------------------------------------------------------------- 3. loop controls
def test_iteration_cap_equals_the_oracle(dot_order):
    ref = reference("rect771x257", 0.5, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4
    got = solve(system("rect771x257"), 0.5, _lib.RULE_CSHARP, 0.0, max_it=3)
    assert_equal_runs(got, ref)
    assert got["messages"] == [maxit_message("MgcgSolveLsqr", got, 3, residual="normal residual")]


def test_min_iteration_beyond_convergence(dot_order):
    s = system("banded1900x700")
    tol = 1e-6 * g0_of(s)
    free = reference("banded1900x700", 0.0, _lib.RULE_CSHARP, tol)
    held = reference("banded1900x700", 0.0, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 6
    assert_equal_runs(solve(s, 0.0, _lib.RULE_CSHARP, tol, min_it=free["iteration"] + 6), held)


def test_a_trace_shorter_than_the_run(dot_order):
    s = system("rect771x257")
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = dict(reference("rect771x257", 0.0, _lib.RULE_CSHARP, tol))
    assert ref["iteration"] + 1 > 5
    ref["trace"] = ref["trace"][:5]
    assert_equal_runs(solve(s, 0.0, _lib.RULE_CSHARP, tol, trace_capacity=5), ref)


def test_garbage_in_the_work_space_and_in_x_does_not_reach_the_result(dot_order):
    """NaN in x and in all six work vectors (u, q by rows; v, w, t by columns)."""
    s = system("rect257x771")
    tol = tolerance(s, _lib.RULE_CSHARP)
    by_rows, by_columns = np.full(s.Rows, np.nan), np.full(s.Columns, np.nan)

    def prepare(cg):
        for v in (cg.vectorU, cg.vectorQ):
            v.CopyFrom(by_rows, s.Rows)
        for v in (cg.vectorX, cg.vectorV, cg.vectorW, cg.vectorT):
            v.CopyFrom(by_columns, s.Columns)

    assert_equal_runs(solve(s, 0.5, _lib.RULE_CSHARP, tol, prepare=prepare), reference("rect257x771", 0.5, _lib.RULE_CSHARP, tol))


@pytest.mark.parametrize("which", ["banded700x1900", "banded1900x700", "convdiff12x10x8"])
def test_every_compression_mode_gives_the_mode_0_bits(dot_order, which):
    """The banded matrices have few distinct rows-as-sequences, so the lossless forms apply -- to A and to A^T each by itself (the tall one
    of each pair must not take the row-pattern form)."""
    s = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    runs = [solve(s, 0.0, _lib.RULE_CSHARP, tol, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert_equal_runs(runs[0], reference(which, 0.0, _lib.RULE_CSHARP, tol))
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


@pytest.mark.parametrize("which", ["rect257x771", "banded1900x700", "rect1900x700x40"])
def test_initialize_forms_the_transpose_of_the_contract(which):
    s = system(which)
    want = transpose_arrays(s.Elements, s.ColumnIndeces, s.RowOffsets, s.Columns)
    seen = {}
    solve(s, 0.0, _lib.RULE_CSHARP, 0.0, max_it=0, inspect=lambda cg: seen.update(at=cg.transpose_arrays()))
    e, c, ro = seen["at"]
    assert e.tobytes() == want[0].tobytes() and np.array_equal(c, want[1]) and np.array_equal(ro, want[2])


def test_a_matrix_the_transposition_refuses_raises_in_initialize():
    s = system("rect771x257")
    bad = problems.least_squares(s, s.Columns - 1)                   # some row stores column 256 of a matrix that now has 256
    cg = LeastSquaresGpu(bad.Rows, bad.Columns, 16, 0, 10, 1e-8).load(bad)
    with pytest.raises(_lib.MgcgError, match="stores column"):
        cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    cg.Dispose()


# --------------------------------------------------------------------------- 4. default mode
# 100 x the largest || x - x_oracle || / || x_oracle || of the first run on an MI355X (1.286e-11, convdiff12x10x8: the docstring below has
# all eight); it may not exceed 1e-8
DEFAULT_MODE_LIMIT = 1.286e-9


@pytest.mark.parametrize("which", NOT_EXHAUSTED)
def test_default_dot_order_solves_to_the_stop_level(which):
    """Every solve stops at 1e-10 relative in g.  TrueNormalResidual <= 2 x the stop level is a condition, not a measurement: the oracle
    alone has the true figure equal to g to three digits on these cases (tests/test_lsqr_host.py).  The distance to the oracle's x is
    bounded by DEFAULT_MODE_LIMIT = 100 x the largest distance of the first run on the GPU (printed per case below), and never more than
    1e-8: with condition numbers up to 110 and a 1e-10 stop anything larger is a defect, not summation order.
    First run (bodies equal to the oracle's in every case; TrueNormalResidual / stop level; distance):
        rect771x257       53   0.848   4.245e-14        banded1900x700     29   0.520   8.474e-16
        rect257x771       85   0.846   7.282e-12        banded700x1900     16   0.190   3.811e-16
        rect1900x700x40   51   0.719   8.416e-16        convdiff12x10x8   177   0.881   1.286e-11
        rect700x1900     170   0.958   1.084e-11        nonsym1037        131   0.995   1.115e-11"""
    s = system(which)
    tol = tolerance(s, _lib.RULE_CSHARP)
    ref = reference(which, 0.0, _lib.RULE_CSHARP, tol)
    got = solve(s, 0.0, _lib.RULE_CSHARP, tol)
    distance = float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    print(f"DEFAULT_MODE {which}: bodies {got['iteration']} (oracle {ref['iteration']}), g {got['residual']:.3e}, TrueNormalResidual "
          f"{got['true_normal_residual']:.3e} = {got['true_normal_residual'] / tol:.3f} x the stop level, distance {distance:.3e}")
    assert DEFAULT_MODE_LIMIT <= 1e-8
    assert got["status"] == ref["status"] == _lib.OK
    assert got["true_normal_residual"] <= 2.0 * tol
    assert distance <= DEFAULT_MODE_LIMIT


# --------------------------------------------------------------------------- 5. breakdowns
def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0(dot_order):
    s = system("rect771x257")
    zero = problems.least_squares(s, s.Columns, np.zeros(s.Rows), "b0")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        ref = lsqr_oracle(zero, 0.0, rule, 1e-12)
        assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0
        got = solve(zero, 0.0, rule, 1e-12)
        assert_equal_runs(got, ref)
        assert got["messages"] == [nonfinite_message("MgcgSolveLsqr", got, NONFINITE_BETA)]


def test_a_right_hand_side_orthogonal_to_the_range_gives_nonfinite_at_iteration_0(dot_order):
    s = system("banded1900x700")
    orth = problems.least_squares(s, s.Columns, orthogonal_rhs(s), "b-orthogonal")
    ref = lsqr_oracle(orth, 0.0, _lib.RULE_CSHARP, 1e-12)
    assert ref["status"] == _lib.NONFINITE and ref["iteration"] == 0 and ref["true_normal_residual"] == 0.0
    got = solve(orth, 0.0, _lib.RULE_CSHARP, 1e-12)
    assert_equal_runs(got, ref)
    assert got["messages"] == [nonfinite_message("MgcgSolveLsqr", got, NONFINITE_ALPHA)]


@pytest.mark.parametrize("serial", [False, True], ids=["default", "dot_order"])
def test_the_exhausted_300_by_7_case_ends_ok(mgcg_env, serial):
    if serial:
        mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    s = system("rect300x7")
    tol = tolerance(s, _lib.RULE_CSHARP)
    got = solve(s, 0.0, _lib.RULE_CSHARP, tol)
    assert got["status"] == _lib.OK and got["iteration"] <= 8 and got["messages"] == []
    assert got["true_normal_residual"] <= tol
