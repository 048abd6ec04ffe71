"""Mixed-precision CG on the GPU (MgcgMixedSetup, CsrMVFloat, SolveMixed, mixed.ConjugateGradientMixedGpu).

The yardstick is ``mixed_cg_oracle`` of tests/test_mixed_host.py: the loop of include/MgcgGpu.h in np.float32 / np.float64 with serial
sums.  Under dot_order = 1 the HIP loop must EQUAL it -- trace, x, r, iteration, residual, status and the number of reliable updates;
in the default mode only the summation order of the dots (and of long rows) differs, and the method's promise is tested instead: an
independent fp64 residual below the tolerance in about the same number of iterations.

Tolerances are relative: ``rel * || b ||`` for the absolute rules, ``rel`` for MGCG_RULE_VIENNACL."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.mixed import ConjugateGradientMixedGpu
from conjugategradient_amd.solver import ApplicationException, VectorDouble
from oracle import oracle as O
from tests.gpu_util import Handles, cap_inside_a_chunk, dvec, ivec, same_under_every_chunking
from tests.test_mixed_host import mixed_cg_oracle, row_sums

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL]
MAX_IT = 600


# --------------------------------------------------------------------------- systems
def with_random_b(s, seed, name):
    b = np.random.default_rng(seed).standard_normal(s.Count)
    return problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count), b, name, s.grid)


def ragged(n=1337, seed=7):
    """The ragged matrix of tests/test_gpu_jacobi.py, rebuilt here: symmetric, rows of 2 .. ~24 entries, unsorted, the diagonal anywhere in
    the row and dominant, no empty rows, a row count that is no multiple of the 256-row tile."""
    rng = np.random.default_rng(seed)
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for j in rng.choice(n, size=rng.integers(1, 12), replace=False):
            j = int(j)
            if j != i:
                v = -rng.random()
                rows[i][j] = v
                rows[j][i] = v
    e, c, r = [], [], [0]
    for i in range(n):
        entries = list(rows[i].items())
        diag = (i, sum(-v for _, v in entries) + 0.5 + 10.0 * rng.random())
        entries.insert(int(rng.integers(0, len(entries) + 1)), diag)
        for j, v in entries:
            c.append(j)
            e.append(v)
        r.append(len(c))
    e, c, r = np.array(e), np.array(c, dtype=np.int32), np.array(r, dtype=np.int32)
    assert n % 256 != 0 and (np.diff(r) > 0).all()
    b = np.cos(np.arange(n) * 0.3) * (1.0 + np.arange(n) % 5)
    return problems.LinearSystem(e, c, r, np.zeros(n), b, "ragged")


def tridiagonal(n):
    """Symmetric tridiagonal, -1 off the diagonal, the diagonal 2.5 + (i mod 7) (strictly dominant), b = cos(0.3 i)."""
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    vals = np.stack([-np.ones(n), 2.5 + (i % 7), -np.ones(n)], axis=1)
    keep = (cols >= 0) & (cols < n)
    ro = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return problems.LinearSystem(vals[keep], cols[keep].astype(np.int32), ro, np.zeros(n), np.cos(0.3 * i), "tridiagonal")


def with_empty_row(n=300):
    """A tridiagonal matrix whose row 77 stores nothing (product only: the matrix is singular)."""
    s = tridiagonal(n)
    ro = s.RowOffsets.astype(np.int64)
    a, b = ro[77], ro[78]
    keep = np.ones(s.nnz, dtype=bool)
    keep[a:b] = False
    ro2 = ro.copy()
    ro2[78:] -= b - a
    return problems.LinearSystem(s.Elements[keep], s.ColumnIndeces[keep], ro2.astype(np.int32), s.x, s.b, "empty-row")


def long_rows(width, n=150, seed=3):
    """Rows of exactly `width` positive entries of mixed size in random column order: the lanes-per-row forms of the product."""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.integers(0, n, size=width) for _ in range(n)]).astype(np.int32)
    e = (0.5 + rng.random(n * width)) * 10.0 ** rng.integers(-2, 3, size=n * width)
    ro = (np.arange(n + 1) * width).astype(np.int32)
    return problems.LinearSystem(e, c, ro, np.zeros(n), np.ones(n), "long-rows")


SYSTEMS = {
    "poisson8": lambda: with_random_b(problems.poisson(8, 8, 8), 11, "poisson8"),                # 512 rows: two tiles
    "grid7x9x11": lambda: with_random_b(problems.poisson(7, 9, 11), 12, "grid7x9x11"),          # 693 rows: no multiple of the 256-row tile, odd
    "ragged": ragged,
    "viennacl4000": lambda: problems.viennacl_main(4000),                                        # 160 entries per row: the lanes-per-row form
}
_systems, _oracles = {}, {}


def system(which):
    if which not in _systems:
        _systems[which] = SYSTEMS[which]()
    return _systems[which]


def tolerance(s, rule, rel):
    return rel if rule == _lib.RULE_VIENNACL else rel * float(np.linalg.norm(s.b))


def yardstick(which, rule, rel, min_it=0, x0=None, key=None):
    """The oracle's run, computed once per case and shared."""
    k = (which, rule, rel, min_it, key)
    if k not in _oracles:
        s = system(which)
        _oracles[k] = mixed_cg_oracle(s, rule, tolerance(s, rule, rel), min_it=min_it, max_it=MAX_IT, x0=x0)
    return _oracles[k]


# --------------------------------------------------------------------------- device helpers
def fvec(a):
    """float32 array -> a double Vector read as floats."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    padded = np.zeros(2 * ((len(a) + 1) // 2) or 2, dtype=np.float32)
    padded[: len(a)] = a
    return dvec(padded.view(np.float64))


def read_floats(v, n):
    return v.to_numpy((n + 1) // 2).view(np.float32)[:n].copy()


class DeviceSystem:
    def __init__(self, h, s):
        self.h, self.s, self.n, self.nnz = h, s, s.Count, s.nnz
        self.e, self.c, self.ro = dvec(s.Elements[: s.nnz]), ivec(s.ColumnIndeces[: s.nnz]), ivec(s.RowOffsets)
        self.e32 = VectorDouble(max((s.nnz + 1) // 2, 1))
        self.exact = None

    def setup(self):
        exact = C.c_int(-1)
        st = _lib.lib().MgcgMixedSetup(self.h.sparse, self.e.Ptr, self.ro.Ptr, self.c.Ptr, self.nnz, self.n, self.e32.Ptr, C.byref(exact))
        self.exact = exact.value
        return st

    def product(self, x32):
        vx, vy = fvec(x32), fvec(np.full(self.n, 7.0, dtype=np.float32))
        _lib.lib().CsrMVFloat(self.h.sparse, self.h.descr, vy.ToRawPtr(), self.e32.ToRawPtr(), self.ro.ToRawPtr(), self.c.ToRawPtr(), vx.ToRawPtr(), self.nnz, self.n)
        _lib.check("CsrMVFloat")
        return read_floats(vy, self.n)

    def solve(self, rule, tol, min_it=0, max_it=MAX_IT, x0=None, e32=None):
        s, n = self.s, self.n
        vx = dvec(s.x if x0 is None else x0)
        vb, vAp, vp, vr = dvec(s.b), dvec(np.zeros(n)), dvec(np.zeros(n)), dvec(np.zeros(n))
        it, res, up = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
        cap = max(max_it, min_it) + 8
        tr = np.zeros(cap)
        st = _lib.lib().SolveMixed(self.h.blas, self.h.sparse, self.h.descr, self.e.Ptr, self.ro.Ptr, self.c.Ptr, vx.Ptr, vb.Ptr, vAp.Ptr, vp.Ptr, vr.Ptr,
                                   (self.e32 if e32 is None else e32).Ptr, self.nnz, n, tol, min_it, max_it, rule,
                                   C.byref(it), C.byref(res), C.byref(up), tr.ctypes.data_as(C.c_void_p), cap)
        msg = _lib.last_error()
        _lib.lib().MgcgClearLastError()
        return dict(status=st, iteration=it.value, residual=res.value, updates=up.value, trace=tr[: max(it.value, 0) + 1].copy(), x=vx.to_numpy(n), r=vr.to_numpy(n),
                    message=msg)


@pytest.fixture(scope="module")
def h():
    handles = Handles()
    yield handles
    handles.close()


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"], got["message"]
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert got["updates"] == ref["updates"], (got["updates"], ref["updates"])
    assert got["residual"] == ref["residual"]
    assert np.array_equal(got["trace"], ref["trace"])
    assert np.array_equal(got["x"], ref["x"])
    assert np.array_equal(got["r"], ref["r"])


# --------------------------------------------------------------------------- 1. set-up
def test_setup_converts_bit_for_bit_and_reports_exactness(h):
    for which, exact in (("poisson8", 1), ("viennacl4000", 0)):
        s = system(which)
        d = DeviceSystem(h, s)
        assert d.setup() == 0 and d.exact == exact, (which, d.exact)
        got = read_floats(d.e32, s.nnz)
        assert got.tobytes() == s.Elements[: s.nnz].astype(np.float32).tobytes()


def test_setup_names_the_first_row_beyond_the_float_range_and_no_solve_runs(h):
    s = system("grid7x9x11")
    e = s.Elements[: s.nnz].copy()
    e[int(s.RowOffsets[600]) + 1] = -1e39
    e[int(s.RowOffsets[411])] = 1e39
    e[int(s.RowOffsets[500]) + 2] = np.inf
    d = DeviceSystem(h, problems.LinearSystem(e, s.ColumnIndeces, s.RowOffsets, s.x, s.b, "beyond", s.grid))
    assert d.setup() == -1
    msg = _lib.last_error()
    _lib.lib().MgcgClearLastError()
    assert "MgcgMixedSetup: row 411 " in msg, msg
    # the Python class raises in Initialize(), before any solve
    cg = ConjugateGradientMixedGpu(s.Count, 7, 0, 50, 1e-8).load(d.s)
    with pytest.raises(_lib.MgcgError, match="row 411 "):
        cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    cg.Dispose()


# --------------------------------------------------------------------------- 2. the fp32 product
def serial_product(s, x32):
    return row_sums(s.Elements[: s.nnz].astype(np.float32), s.ColumnIndeces[: s.nnz], s.RowOffsets, x32)


def _x32(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("which", ["poisson8", "grid7x9x11", "one-row", "empty-row", "ragged"])
def test_product_equals_the_serial_float32_product(h, which):
    if which == "one-row":
        s = problems.LinearSystem(np.array([3.25]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.zeros(1), np.ones(1), "one-row")
    elif which == "empty-row":
        s = with_empty_row()
    else:
        s = system(which)
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    x = _x32(s.Count)
    got = d.product(x)
    assert np.array_equal(got, serial_product(s, x))
    if which == "empty-row":
        assert got[77] == 0.0 and not np.signbit(got[77])


@pytest.mark.parametrize("which", ["ragged_spd1350", "poisson20x17x13"])
def test_product_drops_the_products_of_masked_slots(h, which):
    """inf, -inf, nan and the largest float in x (tests/block_cases.py: poison): the serial float32 product's values, NaN where it has NaN,
    and every row that stores none of those columns finite.  Both matrices take the lane = row form (mean row length below 20)."""
    from tests.block_cases import assert_poisoned_product, poison, ragged_spd

    s = ragged_spd(1350) if which == "ragged_spd1350" else problems.poisson(20, 17, 13)
    assert s.nnz <= 20 * s.Count
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    x = _x32(s.Count)
    clean = poison(s, x)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = serial_product(s, x)
    assert_poisoned_product(d.product(x), ref, clean)


@pytest.mark.parametrize("width", [24, 100, 300])       # 8, 16 and 32 lanes per row
def test_long_rows_take_the_lanes_per_row_form(h, mgcg_env, width):
    """Positive terms, so that the rounding of a `width`-term float32 sum in any order is width * 2^-24 relative to the row's value."""
    s = long_rows(width)
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    x = np.abs(_x32(s.Count)) + np.float32(0.25)
    ref = serial_product(s, x)
    got = d.product(x)
    assert not np.array_equal(got, ref)                               # another summation order: not the lane = row form
    np.testing.assert_allclose(got, ref, rtol=width * 2.0 ** -24, atol=0.0)
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    assert np.array_equal(d.product(x), ref)
    mgcg_env.delenv("MGCG_DOT_ORDER")


# --------------------------------------------------------------------------- 3. dot_order = 1: equal to the yardstick
@pytest.mark.parametrize("rel", [1e-8, 1e-12])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_solve_mixed_equals_the_yardstick_bit_for_bit(h, dot_order, which, rule, rel):
    s = system(which)
    ref = yardstick(which, rule, rel)
    assert ref["status"] == _lib.OK and ref["updates"] >= 2
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    got = d.solve(rule, tolerance(s, rule, rel))
    print(which, rule, rel, "iterations", got["iteration"], ref["iteration"], "updates", got["updates"], ref["updates"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("which", ["grid7x9x11", "ragged"])
def test_min_iteration_and_initial_guess_equal_the_yardstick(h, dot_order, which):
    s = system(which)
    x0 = np.sin(np.arange(s.Count) * 0.7) * 3.0
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    for rule in (_lib.RULE_CSHARP, _lib.RULE_SIMPLE):
        plain = yardstick(which, rule, 1e-8)
        min_it = plain["iteration"] + 6
        ref = yardstick(which, rule, 1e-8, min_it=min_it)
        assert ref["iteration"] >= min_it > plain["iteration"]
        assert_equal_runs(d.solve(rule, tolerance(s, rule, 1e-8), min_it=min_it), ref)
    ref = yardstick(which, _lib.RULE_NATIVE, 1e-12, x0=x0, key="x0")
    assert not np.array_equal(ref["x"], yardstick(which, _lib.RULE_NATIVE, 1e-12)["x"])
    assert_equal_runs(d.solve(_lib.RULE_NATIVE, tolerance(s, _lib.RULE_NATIVE, 1e-12), x0=x0), ref)
    # MGCG_RULE_SIMPLE ignores the guess
    assert_equal_runs(d.solve(_lib.RULE_SIMPLE, tolerance(s, _lib.RULE_SIMPLE, 1e-8), x0=x0), yardstick(which, _lib.RULE_SIMPLE, 1e-8))


# --------------------------------------------------------------------------- 4. the default mode
@pytest.mark.parametrize("rel", [1e-8, 1e-12])
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_default_mode_reaches_the_tolerance_on_an_independent_residual(h, which, rel):
    s = system(which)
    rule = _lib.RULE_CSHARP
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    got = d.solve(rule, tolerance(s, rule, rel))
    again = d.solve(rule, tolerance(s, rule, rel))
    assert got["status"] == _lib.OK, got["message"]
    normb = float(np.linalg.norm(s.b))
    independent = float(np.linalg.norm(s.b - O.spmv(s.Elements[: s.nnz], s.ColumnIndeces[: s.nnz], s.RowOffsets, got["x"]))) / normb
    ref = yardstick(which, rule, rel)
    print(which, rel, "independent residual", independent, "reported", got["residual"] / normb, "iterations", got["iteration"], "dot_order = 1:", ref["iteration"],
          "updates", got["updates"])
    assert independent < 2 * rel
    assert got["residual"] < rel * normb and got["iteration"] % 4 == 3
    assert abs(got["iteration"] - ref["iteration"]) <= 2
    for k in ("x", "r", "trace"):
        assert got[k].tobytes() == again[k].tobytes(), k
    assert (got["iteration"], got["residual"], got["updates"], got["status"]) == (again["iteration"], again["residual"], again["updates"], again["status"])


# --------------------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("max_it", [9, 7])       # 7: the worst slot delay, the cap is noticed in iteration 8 and reported in iteration 11 = max_it + 4
def test_iteration_cap_reports_a_true_residual(h, dot_order, max_it):
    s = system("grid7x9x11")
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    ref = mixed_cg_oracle(s, _lib.RULE_CSHARP, 0.0, max_it=max_it)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 11       # the first update slot behind the cap
    got = d.solve(_lib.RULE_CSHARP, 0.0, max_it=max_it)
    assert_equal_runs(got, ref)
    # "SolveMixed: did not converge: iteration 11 exceeded maxIteration 9 (true residual ...)"
    assert got["message"] == "SolveMixed: did not converge: iteration %d exceeded maxIteration %d (true residual %g)" % (got["iteration"], max_it, got["residual"])
    true_r = s.b - O.spmv(s.Elements[: s.nnz], s.ColumnIndeces[: s.nnz], s.RowOffsets, got["x"])
    assert np.array_equal(got["r"], true_r) and got["residual"] == math.sqrt(O.dot(true_r, true_r))


def indefinite():
    """Poisson 8^3 with the sign of one diagonal entry flipped (and made large): p.Ap turns negative within a few iterations."""
    s = system("poisson8")
    e = s.Elements[: s.nnz].copy()
    row = 200
    k = int(s.RowOffsets[row]) + int(np.nonzero(s.ColumnIndeces[s.RowOffsets[row]: s.RowOffsets[row + 1]] == row)[0][0])
    e[k] = -60.0
    return problems.LinearSystem(e, s.ColumnIndeces, s.RowOffsets, s.x, s.b, "indefinite", s.grid)


def test_an_indefinite_matrix_breaks_down_with_a_finite_x(h):
    bad = indefinite()
    d = DeviceSystem(h, bad)
    assert d.setup() == 0
    got = d.solve(_lib.RULE_CSHARP, 1e-10 * float(np.linalg.norm(bad.b)), max_it=300)
    assert got["status"] == _lib.NONFINITE, (got["status"], got["iteration"])
    assert got["message"] == ("SolveMixed: stopped at iteration %d: p.Ap is not finite and > 0, or the residual is not finite or beyond the fp32 range"
                              % got["iteration"]) and np.isfinite(got["x"]).all()


@pytest.mark.parametrize("first_ok", [0, 5])
def test_breakdown_keeps_the_last_folded_iterate_and_true_residual(h, dot_order, first_ok):
    """What the header promises of a breakdown, against the yardstick: x at its last folded iterate, r the last true residual, the trace
    entry and the residual of the recurrence.  first_ok = 5: the entry is flipped in a matrix copy whose first iterations are Poisson's
    (the row's right-hand side and neighbours are 0 until the recurrence reaches it), so an update has folded x before the breakdown."""
    bad = indefinite()
    if first_ok:
        b = bad.b.copy()
        b[np.abs(np.arange(bad.Count) - 200) < 150] = 0.0       # row 200 is reached only after a few iterations
        bad = problems.LinearSystem(bad.Elements, bad.ColumnIndeces, bad.RowOffsets, bad.x, b, "indefinite-late", bad.grid)
    tol = 1e-10 * float(np.linalg.norm(bad.b))
    ref = mixed_cg_oracle(bad, _lib.RULE_CSHARP, tol, max_it=300)
    assert ref["status"] == _lib.NONFINITE
    if first_ok:
        assert ref["updates"] >= 1 and ref["x"].any(), (ref["iteration"], ref["updates"])
    d = DeviceSystem(h, bad)
    assert d.setup() == 0
    got = d.solve(_lib.RULE_CSHARP, tol, max_it=300)
    print("breakdown at iteration", got["iteration"], "updates", got["updates"])
    assert_equal_runs(got, ref)
    assert np.isfinite(got["x"]).all()


def test_refused_calls_enqueue_nothing(h):
    s = system("poisson8")
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    x0 = np.arange(s.Count) * 0.25 + 1.0
    got = d.solve(_lib.RULE_HANDMADECL, 1e-8, x0=x0)
    assert got["status"] == _lib.ERROR and "MGCG_RULE_HANDMADECL" in got["message"]
    assert np.array_equal(got["x"], x0) and not got["r"].any()
    small = VectorDouble(max((s.nnz + 1) // 2 - 1, 1))
    got = d.solve(_lib.RULE_CSHARP, 1e-8, x0=x0, e32=small)
    assert got["status"] == _lib.ERROR and "elements32" in got["message"]
    assert np.array_equal(got["x"], x0) and not got["r"].any()


@pytest.mark.parametrize("n", [5, 1021, 1022, 1023])       # n mod 4 = 1, 1, 2, 3; one quad, and 255 quads
def test_row_counts_that_are_no_multiple_of_four_take_the_element_wise_tail(h, dot_order, n):
    s = tridiagonal(n)
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    tol = 1e-12 * float(np.linalg.norm(s.b))
    assert_equal_runs(d.solve(_lib.RULE_NATIVE, tol), mixed_cg_oracle(s, _lib.RULE_NATIVE, tol, max_it=MAX_IT))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_rows_than_a_quad_equal_the_yardstick(h, dot_order, n):
    """No quad at all: one workgroup, the tail lanes only.  Such systems are solved exactly between two update slots, after which p.Ap is
    0 or noise, so the runs end as they may (n = 1: a breakdown in iteration 1); whatever the yardstick does, the HIP loop does."""
    s = tridiagonal(n)
    tol = 1e-12 * float(np.linalg.norm(s.b))
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    ref = mixed_cg_oracle(s, _lib.RULE_NATIVE, tol, max_it=40)
    got = d.solve(_lib.RULE_NATIVE, tol, max_it=40)
    print(n, "status", got["status"], ref["status"], "iteration", got["iteration"], ref["iteration"])
    assert_equal_runs(got, ref)


# --------------------------------------------------------------------------- 6. the streaming-hint forms
STREAMING_ROWS = 3_000_001      # the smallest row count at which the vector passes take their streaming-hint forms (n > 3 000 000); odd: the tail runs


def test_streaming_hint_forms_equal_the_yardstick(h, dot_order):
    """Eight forced iterations (tolerance 0, cap 6: the update slot of iteration 7 reports the cap), two reliable updates."""
    s = tridiagonal(STREAMING_ROWS)
    ref = mixed_cg_oracle(s, _lib.RULE_CSHARP, 0.0, max_it=6)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 7 and ref["updates"] == 2, (ref["status"], ref["iteration"], ref["updates"])
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    assert_equal_runs(d.solve(_lib.RULE_CSHARP, 0.0, max_it=6), ref)


# --------------------------------------------------------------------------- 7. the class surface
def test_class_gives_the_raw_call_s_bits(h):
    s = system("ragged")
    rule, tol = _lib.RULE_CSHARP, tolerance(system("ragged"), _lib.RULE_CSHARP, 1e-12)
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    raw = d.solve(rule, tol)
    cg = ConjugateGradientMixedGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, MAX_IT, tol, rule=rule).load(s)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    assert cg.Exact is False and cg.ReliableUpdates == raw["updates"] >= 2
    assert (cg.Iteration, cg.Residual, cg.status) == (raw["iteration"], raw["residual"], _lib.OK)
    assert np.array_equal(cg.x, raw["x"]) and np.array_equal(cg.trace, raw["trace"])
    cg.Dispose()


def test_class_raises_on_maximum_iterations(h):
    s = system("poisson8")
    cg = ConjugateGradientMixedGpu(s.Count, 7, 0, 5, 1e-300).load(s)
    cg.Initialize()
    assert cg.Exact is True
    with pytest.raises(ApplicationException, match="MaxIteration=5"):
        cg.Solve()
    assert cg.status == _lib.MAXIT_EXCEEDED and cg.Iteration == 7
    cg.Dispose()


@pytest.mark.parametrize("order", [0, 1])
def test_chunking_cannot_change_a_result(h, order):
    """check_every = 1, 4, 7 on 8^3 Poisson: the same bits, also when the iteration cap ends the loop in the middle of a chunk."""
    d = DeviceSystem(h, system("poisson8"))
    assert d.setup() == 0
    keys = ("status", "iteration", "residual", "updates", "trace", "x", "r")

    def run(max_it):
        got = d.solve(_lib.RULE_VIENNACL, 1e-8, max_it=max_it)
        return {key: got[key] for key in keys}

    free = same_under_every_chunking(lambda: run(MAX_IT), order)
    print("iteration", free["iteration"], "updates", free["updates"])
    assert free["status"] == _lib.OK and free["iteration"] > 8
    cap = cap_inside_a_chunk(0, free["iteration"])
    capped = same_under_every_chunking(lambda: run(cap), order)
    print("cap", cap, "iteration", capped["iteration"])
    assert capped["status"] == _lib.MAXIT_EXCEEDED and cap < capped["iteration"] <= cap + 4       # (reported at the next update slot)
