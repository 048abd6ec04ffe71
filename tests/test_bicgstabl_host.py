"""BiCGStab(l) on the host side (no GPU needed): the yardstick of tests/test_gpu_bicgstabl.py lives here and is checked against the true
residual, against ``bicgstab_oracle`` on the system that loop cannot solve, and on the corner cases of the method; the library exports the
two entry points and refuses bad arguments before it asks for a device.

``bicgstabl_oracle`` is the loop of include/MgcgGpu.h (SolveBicgstabL / SolveBicgstabLJacobi) in np.float64: every product goes into a named
array or scalar before the add that follows it, a matrix row is summed serially in stored order from +0.0 (``row_sums``), the scalars are
evaluated in the header's order -- the Cholesky factor row by row, the two triangular solves and the three sums of the combine pass term by
term for j = 1 .. l, the stop test on r_0.r_0 in front of steps 1 .. l-1 -- and every sum is a serial left-to-right sum (``serial_sum``).  The loop runs on one rank: ``parts`` is accepted, as
``bicgstab_oracle`` accepts it, and cuts the sums the same way; an empty part changes nothing.  Under dot_order = 1 the HIP loop must EQUAL it.

Systems: 32 x 32 with c = (20, 20, 0) is the one ``bicgstab_oracle`` ends MGCG_NONFINITE on; every case listed here met 1.001 x the stop
level with serial sums, so none was replaced."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_bicgstab_host import bicgstab_oracle, nonsymmetric_tridiagonal, numpy_true_residual, small
from tests.test_mixed_host import row_sums, serial_sum
from tests.test_sreduce_host import diagonal_of, stop_decision, with_b
from tests.test_variant_refusals_host import EIGHT, H, OUT3, SHORT, STOP, TINY, VEC, _VectorHead

DBL_BIG = 1.79e308
ELLS = [1, 2, 3, 4]


# --------------------------------------------------------------------------- the yardstick
def gamma_of(Z, ell):
    """(gamma_1 .. gamma_l, m) from Z[a][b] = r_a.r_b (a = 1 .. l, b = 0 .. a) in the header's scalar order: the Cholesky factor of
    Z[1..l, 1..l] row by row, m leading pivots that are > 0 and finite, the two triangular solves on the leading m x m system."""
    f = np.float64
    Cf = [[f(0.0)] * (ell + 1) for _ in range(ell + 1)]
    m = 0
    for i in range(1, ell + 1):
        for j in range(1, i):
            s = Z[i][j]
            for q in range(1, j):
                t = Cf[i][q] * Cf[j][q]
                s = s - t
            Cf[i][j] = s / Cf[j][j]
        s = Z[i][i]
        for q in range(1, i):
            t = Cf[i][q] * Cf[i][q]
            s = s - t
        if not (s > 0.0 and abs(s) <= DBL_BIG):
            break
        Cf[i][i] = np.sqrt(s)
        m = i
    y = [f(0.0)] * (ell + 1)
    for i in range(1, m + 1):
        s = Z[i][0]
        for q in range(1, i):
            t = Cf[i][q] * y[q]
            s = s - t
        y[i] = s / Cf[i][i]
    g = [f(0.0)] * (ell + 1)
    for i in range(m, 0, -1):
        s = y[i]
        for q in range(i + 1, m + 1):
            t = Cf[q][i] * g[q]
            s = s - t
        g[i] = s / Cf[i][i]
    return g, m


def bicgstabl_oracle(s, ell, dinv=None, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, parts=None, x0=None, total=serial_sum, step_test=True):
    """A x = s.b from s.x (x0), right-preconditioned with diag(1 / dinv) when dinv is given.  total(terms): the sum of the terms (default:
    serial, left to right).  step_test=False: WITHOUT the stop test in front of steps 1 .. l-1 -- not the library's loop; it is there to show
    what that test is for.  Returns bicgstab_oracle's dict, and ``pivots``: the smallest m any body's factorisation kept."""
    assert 1 <= ell <= 4
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    parts = [0, s.Count] if parts is None else [int(v) for v in parts]
    f = np.float64

    def sums(terms):
        acc = 0.0
        for lo, hi in zip(parts[:-1], parts[1:]):
            acc += total(terms[lo:hi]) if hi > lo else 0.0
        return f(acc)

    def finite(v):
        return bool(abs(v) <= DBL_BIG)

    def hat(v):
        return v if dinv is None else dinv * v

    def product(v):
        return row_sums(e, c, ro, hat(v))

    least = [ell]

    def closing(x, it, res, status, trace):
        r = b - row_sums(e, c, ro, x)
        with np.errstate(all="ignore"):
            true = float(np.sqrt(sums(r * r)))
        return dict(x=x, r=r, iteration=it, residual=res, true_residual=true, status=status, trace=np.array(trace), pivots=least[0])

    with np.errstate(all="ignore"):
        x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
        r = [None] * (ell + 1)
        u = [None] * (ell + 1)
        r[0] = b - row_sums(e, c, ro, x)
        rt = r[0].copy()
        u[0] = r[0].copy()
        rho = rr0 = sums(r[0] * r[0])
        res = float(np.sqrt(rr0))
        shown = float(np.sqrt(rr0 / rr0)) if rule == _lib.RULE_VIENNACL else res
        trace = [shown]
        if not (0.0 < rr0 <= DBL_BIG):
            return closing(x, 0, res, _lib.NONFINITE, trace)
        alpha = f(0.0)
        k = 0
        while True:
            rho1 = None
            for j in range(ell):
                if j > 0:                                                      # pass U_j: the stop test on r_0 as step j - 1 left it, then beta
                    early = stop_decision(rule, tol, min_it, max_it, k + 1, sums(r[0] * r[0]), rr0)
                    if step_test and early[2] and early[3] == _lib.OK:                       # the body ends here; an exceeded cap or a value that is not finite waits for the body's end
                        trace.append(early[1])
                        return closing(x, k + 1, early[0], _lib.OK, trace)
                    ratio = rho1 / rho
                    beta = alpha * ratio
                    rho = rho1
                    for i in range(j + 1):
                        bu = beta * u[i]
                        u[i] = r[i] - bu
                u[j + 1] = product(u[j])
                sigma = sums(rt * u[j + 1])
                alpha = rho / sigma
                if sigma == 0.0 or not finite(sigma) or not finite(alpha):      # breakdown in front of step j's updates: the last judged figure again
                    trace.append(shown)
                    return closing(x, k + 1, res, _lib.NONFINITE, trace)
                h0 = hat(u[0])                                                  # pass R_j
                ah = alpha * h0
                x = x + ah
                for i in range(j + 1):
                    au = alpha * u[i + 1]
                    r[i] = r[i] - au
                r[j + 1] = product(r[j])
                rho1 = sums(rt * r[j + 1])
            Z = [[None] * (ell + 1) for _ in range(ell + 1)]                    # the Gram pass
            for a in range(1, ell + 1):
                for bb in range(a + 1):
                    Z[a][bb] = sums(r[a] * r[bb])
            g, m = gamma_of(Z, ell)
            least[0] = min(least[0], m)
            omega = g[ell]
            u0, xn, r0 = u[0], x, r[0]                                          # the combine pass
            for j in range(1, ell + 1):
                t = g[j] * u[j]
                u0 = u0 - t
            for j in range(1, ell + 1):
                t = g[j] * hat(r[j - 1])
                xn = xn + t
            for j in range(1, ell + 1):
                t = g[j] * r[j]
                r0 = r0 - t
            u[0], x, r[0] = u0, xn, r0
            rr = sums(r0 * r0)
            rhon = sums(rt * r0)
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, rr, rr0)
            trace.append(shown)
            if not stop and (omega == 0.0 or rhon == 0.0 or not finite(rhon)):  # x IS this body's iterate
                stop, status = True, _lib.NONFINITE
            if stop:
                return closing(x, k + 1, res, status, trace)
            mo = -omega                                                         # pass P
            den = mo * rho
            q = rhon / den
            beta = alpha * q
            rho = rhon
            bu = beta * u[0]
            u[0] = r[0] - bu
            k += 1


# --------------------------------------------------------------------------- the systems
SEED = 20261019
MATRICES = {
    "convdiff16": lambda: problems.convection_diffusion(16, 16, 16, (0.5, 0.25, 0.0)),
    "convdiff32x32_5": lambda: problems.convection_diffusion(32, 32, 1, (5.0, 5.0, 0.0)),
    "convdiff32x32_20": lambda: problems.convection_diffusion(32, 32, 1, (20.0, 20.0, 0.0)),
    "convdiff15x15x3": lambda: problems.convection_diffusion(15, 15, 3, (5.0, 5.0, 5.0)),
    "upwind16": lambda: problems.convection_diffusion(16, 16, 16, (2.0, 1.0, 0.5), upwind=True),
    "random_nonsymmetric4097": lambda: problems.random_nonsymmetric(4097, 9, SEED),
    "poisson16": lambda: problems.poisson(16, 16, 16),
}
MIN_ELL = {"convdiff32x32_20": 2}                                                 # l = 1 is BiCGStab, which breaks down there
CASES = [(m, rhs, ell) for m in MATRICES for rhs in ("ones", "randn") for ell in ELLS if ell >= MIN_ELL.get(m, 1)]
MAX_IT = 3000
_systems, _runs = {}, {}


def _product(s, v):
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * v[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


def system(name, rhs="ones"):
    """(system, dinv): the matrix with b = A.1 ("ones") or an N(0,1) b of fixed seed ("randn"), x = 0, and 1 / diag(A)."""
    key = (name, rhs)
    if key not in _systems:
        s = MATRICES[name]()
        b = _product(s, np.ones(s.Count)) if rhs == "ones" else np.random.default_rng(SEED).standard_normal(s.Count)
        s = with_b(s, b, f"{name}-{rhs}")
        _systems[key] = (s, 1.0 / diagonal_of(s))
    return _systems[key]


def run(name, rhs, ell, jacobi, rel=1e-8):
    """The yardstick's run to a relative ``rel`` with serial sums, computed once and shared (nothing changes it)."""
    key = (name, rhs, ell, jacobi, rel)
    if key not in _runs:
        s, dinv = system(name, rhs)
        _runs[key] = bicgstabl_oracle(s, ell, dinv if jacobi else None, _lib.RULE_CSHARP, rel * float(np.linalg.norm(s.b)), max_it=MAX_IT)
    return _runs[key]


def level_of(s, rel=1e-8):
    return rel * float(np.linalg.norm(s.b))


# --------------------------------------------------------------------------- the method
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name,rhs,ell", CASES)
def test_the_true_residual_is_within_the_stop_level(name, rhs, ell, jacobi):
    s, _ = system(name, rhs)
    level = level_of(s)
    o = run(name, rhs, ell, jacobi)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs} l={ell} jacobi={jacobi}: {o['iteration']} bodies = {2 * ell * o['iteration']} products, recurrence {o['residual']:.3e}, "
          f"true {true:.3e} = {true / level:.4f} x the stop level")
    assert o["status"] == _lib.OK
    assert o["residual"] < level
    assert true <= 1.001 * level
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


def test_the_capability_bicgstab_breaks_down_where_ell_2_and_4_converge():
    s, _ = system("convdiff32x32_20", "ones")
    level = level_of(s)
    old = bicgstab_oracle(s, None, _lib.RULE_CSHARP, level, max_it=MAX_IT)
    print(f"bicgstab_oracle: status {old['status']} at body {old['iteration']}, true residual {numpy_true_residual(s, old['x']) / level:.3e} x the level")
    assert old["status"] == _lib.NONFINITE
    for ell in (2, 4):
        o = run("convdiff32x32_20", "ones", ell, False)
        true = numpy_true_residual(s, o["x"])
        print(f"l = {ell}: {o['iteration']} bodies = {2 * ell * o['iteration']} products, true residual {true / level:.4f} x the level")
        assert o["status"] == _lib.OK and true <= 1.001 * level


@pytest.mark.parametrize("name", ["convdiff32x32_5", "convdiff15x15x3"])
def test_ell_2_needs_fewer_products_than_bicgstab(name):
    s, _ = system(name, "ones")
    old = bicgstab_oracle(s, None, _lib.RULE_CSHARP, level_of(s), max_it=MAX_IT)
    new = run(name, "ones", 2, False)
    print(f"{name}: BiCGStab {2 * old['iteration']} products, BiCGStab(2) {4 * new['iteration']}")
    assert old["status"] == new["status"] == _lib.OK
    assert 4 * new["iteration"] < 2 * old["iteration"]


@pytest.mark.parametrize("ell", ELLS)
def test_jacobi_needs_fewer_bodies_on_an_uneven_diagonal_and_the_same_on_a_uniform_one(ell):
    for rhs in ("ones", "randn"):
        plain, jacobi = run("random_nonsymmetric4097", rhs, ell, False), run("random_nonsymmetric4097", rhs, ell, True)
        print(f"random_nonsymmetric4097 {rhs} l={ell}: plain {plain['iteration']} bodies, Jacobi {jacobi['iteration']}")
        assert jacobi["iteration"] < plain["iteration"]
    # a uniform diagonal d = 4, a power of two: M = d I scales hat(.) and 1 / alpha, 1 / gamma alike and nothing else moves
    s, dinv = system("convdiff32x32_5", "randn")
    assert (dinv == 0.25).all()
    plain, jacobi = run("convdiff32x32_5", "randn", ell, False), run("convdiff32x32_5", "randn", ell, True)
    assert jacobi["iteration"] == plain["iteration"] and np.array_equal(jacobi["x"], plain["x"])
    for name in ("convdiff16", "poisson16"):                                       # d = 6: the same up to rounding
        assert abs(run(name, "randn", ell, True)["iteration"] - run(name, "randn", ell, False)["iteration"]) <= 1


# --------------------------------------------------------------------------- rules, start, minimum, cap
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule, ell):
    s, _ = system("convdiff16", "randn")
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else level_of(s)
    o = bicgstabl_oracle(start, ell, None, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 3
    zero = bicgstabl_oracle(s, ell, None, rule, tol, max_it=MAX_IT)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert (o["iteration"] == zero["iteration"] and np.array_equal(o["x"], zero["x"])) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2] and zero["trace"][0] == 1.0
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]


@pytest.mark.parametrize("ell", ELLS)
def test_the_iteration_cap_and_the_minimum_are_kept(ell):
    s, _ = system("convdiff16", "randn")
    capped = bicgstabl_oracle(s, ell, None, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    tol = 1e-2 * float(np.linalg.norm(s.b))
    free = bicgstabl_oracle(s, ell, None, tol=tol, max_it=400)
    held = bicgstabl_oracle(s, ell, None, tol=tol, min_it=free["iteration"] + 3, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 3


@pytest.mark.parametrize("ell", ELLS)
def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0(ell):
    s = nonsymmetric_tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = bicgstabl_oracle(with_b(s, np.zeros(50), "b0"), ell, None, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


# --------------------------------------------------------------------------- tiny systems, breakdowns, the truncated factorisation
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_systems_end_cleanly(n, ell, jacobi):
    s = nonsymmetric_tridiagonal(n)
    level = level_of(s)
    o = bicgstabl_oracle(s, ell, 1.0 / diagonal_of(s) if jacobi else None, tol=level)
    true = numpy_true_residual(s, o["x"])
    print(f"n = {n} l = {ell} jacobi={jacobi}: status {o['status']} after {o['iteration']} bodies, pivots kept {o['pivots']}, true residual {true:.3e}")
    assert o["status"] in (_lib.OK, _lib.NONFINITE)
    assert np.isfinite(o["x"]).all()
    if o["status"] == _lib.OK:
        assert true <= 1.001 * level


def test_why_the_stop_test_stands_in_front_of_a_step():
    """[[2, -.5], [-1.5, 2]], b = A.1, l = 3: two BiCG steps exhaust the Krylov space and leave r_0 at 1e-16.  Without the test in front of
    step 2 that step divides rounding errors -- alpha of the order 1e15 -- and moves x by 1e-2 while the recurrence's r_0 stays at rounding
    level: MGCG_OK with a true residual of 8e-2, seven orders above the level.  With the test the body ends where it converged."""
    s = nonsymmetric_tridiagonal(2)
    level = level_of(s)
    without = bicgstabl_oracle(s, 3, None, tol=level, step_test=False)
    true = numpy_true_residual(s, without["x"])
    print(f"without the test: status {without['status']}, recurrence {without['residual']:.3e}, true residual {true:.3e} = {true / level:.3e} x the level")
    assert without["status"] == _lib.OK and without["residual"] < level
    assert 1e-2 < true < 1.0
    with_test = bicgstabl_oracle(s, 3, None, tol=level)
    assert with_test["status"] == _lib.OK and with_test["iteration"] == 1
    assert numpy_true_residual(s, with_test["x"]) <= 1.001 * level
    assert np.allclose(with_test["x"], np.ones(2), rtol=1e-14, atol=0)


def two_cycle():
    """The rotation by 90 degrees, [[0, -1], [1, 0]], with b = (1, 0): u_1 = A b = (0, 1) and sigma = rt.u_1 = 0 in step 0 of body 0, exactly,
    for every l."""
    return small([[0.0, -1.0], [1.0, 0.0]], [1.0, 0.0], "two_cycle", x=[0.0, 0.0])


@pytest.mark.parametrize("ell", ELLS)
def test_sigma_zero_at_step_0_gives_nonfinite_and_the_callers_x_back(ell):
    s = two_cycle()
    o = bicgstabl_oracle(s, ell, None, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], [0.0, 0.0])
    assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0


def test_a_constructed_sigma_zero_at_step_1():
    """A = [[1, 0, -1], [0, 1, 0], [-1, 0, 1]], b = (1, 0, 0), x = 0.  Every number below is a small integer, so the arithmetic is exact:
      step 0: rt = u_0 = r_0 = (1, 0, 0); u_1 = A u_0 = (1, 0, -1); sigma = 1; rho = 1; alpha = 1; x = (1, 0, 0);
              r_0 = (1, 0, 0) - (1, 0, -1) = (0, 0, 1); r_1 = A r_0 = (-1, 0, 1); rho1 = rt.r_1 = -1
      step 1: beta = 1 * (-1 / 1) = -1; u_0 = r_0 + u_0 = (1, 0, 1); u_1 = r_1 + u_1 = (0, 0, 0); u_2 = A u_1 = 0; sigma = rt.u_2 = 0.
    The breakdown leaves x = (1, 0, 0) and r_0 = (0, 0, 1) = b - A x, what step 0 made them: a consistent pair, and the figure of the
    start is repeated."""
    s = small([[1.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 1.0]], [1.0, 0.0, 0.0], "sigma_zero_at_step_1", x=[0.0, 0.0, 0.0])
    for ell in (2, 3, 4):
        o = bicgstabl_oracle(s, ell, None, tol=1e-12)
        assert o["status"] == _lib.NONFINITE and o["iteration"] == 1
        assert np.array_equal(o["x"], [1.0, 0.0, 0.0]) and np.array_equal(o["r"], [0.0, 0.0, 1.0])
        assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0


def test_the_factorisation_is_truncated_when_the_krylov_space_is_exhausted():
    """diag(2, 4) with b = (1, 0), an eigenvector, and l = 1: u_1 = (2, 0), sigma = 2, alpha = 1/2, x = (1/2, 0), r_0 = 0 and r_1 = 0, all exact.
    Z_11 = 0 is no pivot: m = 0 < l, gamma_1 = omega = 0, and rr = 0 meets the stop test before omega is looked at."""
    s = small([[2.0, 0.0], [0.0, 4.0]], [1.0, 0.0], "eigenvector", x=[0.0, 0.0])
    o = bicgstabl_oracle(s, 1, None, tol=1e-12)
    assert o["pivots"] == 0 and o["status"] == _lib.OK and o["iteration"] == 1
    assert np.array_equal(o["x"], [0.5, 0.0]) and o["residual"] == 0.0 and o["true_residual"] == 0.0
    # with tolerance 0 no rule stops, and omega == 0 is the breakdown behind the body's updates
    o = bicgstabl_oracle(s, 1, None, tol=0.0)
    assert o["pivots"] == 0 and o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], [0.5, 0.0])
    # exactly singular: Z of r_1 = r_2 (a Gram matrix with two equal rows) keeps one pivot, and gamma_2 = 0
    f = np.float64
    Z = [[None] * 3, [f(2.0), f(4.0), None], [f(2.0), f(4.0), f(4.0)]]
    g, m = gamma_of(Z, 2)
    assert m == 1 and g[1] == 0.5 and g[2] == 0.0
    # a pivot that is not finite ends it as well
    Z = [[None] * 3, [f(2.0), f(np.inf), None], [f(2.0), f(4.0), f(4.0)]]
    assert gamma_of(Z, 2)[1] == 0
    # and the full case: G = [[4, 2], [2, 5]], rhs (2, 3): C = [[2, 0], [1, 2]], y = (1, 1), gamma = (1/4, 1/2)
    Z = [[None] * 3, [f(2.0), f(4.0), None], [f(3.0), f(2.0), f(5.0)]]
    g, m = gamma_of(Z, 2)
    assert m == 2 and g[1] == 0.25 and g[2] == 0.5


def test_sums_cut_at_parts_are_accepted_and_an_empty_part_changes_nothing():
    s, _ = system("random_nonsymmetric4097", "randn")
    tol = level_of(s)
    one = run("random_nonsymmetric4097", "randn", 2, False)
    cut = bicgstabl_oracle(s, 2, None, tol=tol, max_it=MAX_IT, parts=problems.partition_offsets(s.Count, 3))
    assert cut["status"] == _lib.OK and abs(one["iteration"] - cut["iteration"]) <= 2
    assert numpy_true_residual(s, cut["x"]) <= 1.001 * tol
    empty = bicgstabl_oracle(s, 2, None, tol=tol, max_it=MAX_IT, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- the library's host side
EXPORTS = ("SolveBicgstabL", "SolveBicgstabLJacobi")


def test_both_symbols_are_exported_and_bound(hiplib):
    for name in EXPORTS:
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import bicgstab

    assert "BiCGStab(l)" in conjugategradient_amd.__doc__ and "BiCGStab(l)" in bicgstab.__doc__
    assert issubclass(bicgstab.BiConjugateGradientStabLGpu, bicgstab.BiConjugateGradientStabGpu)
    assert issubclass(bicgstab.BiConjugateGradientStabLJacobiGpu, bicgstab.BiConjugateGradientStabLGpu)
    for cls in (bicgstab.BiConjugateGradientStabLGpu, bicgstab.BiConjugateGradientStabLJacobiGpu):
        cg = cls.__new__(cls)
        cg._ready = False
        with pytest.raises(_lib.MgcgError, match="Initialize"):
            cg.Solve()
        with pytest.raises(ValueError, match="max-norm"):
            cls(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
        with pytest.raises(ValueError, match="max-norm"):
            cls(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL, ell=4)


def _call(L, jacobi, blas=H, sparse=H, work=None, dinv=VEC, ell=2, rule=_lib.RULE_CSHARP, work_size=None):
    """One call with zeroed handles and vector heads of 10 entries: a refused call looks at nothing else.  (status, message)"""
    head = _VectorHead(None, (50 if work_size is None else work_size), -1, b"")
    if work is None:
        work = C.addressof(head)
    elif work == "null":
        work = None
    L.MgcgClearLastError()
    fn = L.SolveBicgstabLJacobi if jacobi else L.SolveBicgstabL
    st = fn(blas, sparse, None, *EIGHT, work, *((dinv,) if jacobi else ()), ell, 28, 10, *STOP, rule, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    return st, msg


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib, jacobi):
    L = hiplib
    who = "SolveBicgstabLJacobi" if jacobi else "SolveBicgstabL"
    for kw in [dict(blas=None), dict(sparse=None), dict(work="null")] + ([dict(dinv=None)] if jacobi else []):
        st, msg = _call(L, jacobi, **kw)
        assert st == _lib.ERROR and msg == f"{who}: null handle", (kw, msg)
    for ell in (0, 5, -1, 17):
        st, msg = _call(L, jacobi, ell=ell)
        assert st == _lib.ERROR and msg == f"{who}: ell = {ell}, must be 1 .. 4", msg
    st, msg = _call(L, jacobi, rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "MGCG_RULE_HANDMADECL" in msg and msg.startswith(f"{who}:")
    for rule in (-1, 5):
        st, msg = _call(L, jacobi, rule=rule)
        assert st == _lib.ERROR and msg == f"{who}: unknown stop rule {rule}"
    # 10 rows: slices of 10 entries, 2 l of them and one more with the diagonal
    for ell in ELLS:
        need = (2 * ell + (1 if jacobi else 0)) * 10
        st, msg = _call(L, jacobi, ell=ell, work_size=need - 1)
        assert st == _lib.ERROR and f"the work vector holds {need - 1} entries" in msg and f"ell = {ell} needs {need}" in msg, msg
    if jacobi:
        st, msg = _call(L, jacobi, dinv=SHORT)
        assert st == _lib.ERROR and "the dinv vector holds 9 entries" in msg
    # ell is looked at before the rule, the rule before the work vector, the work vector before dinv
    assert "ell = 9" in _call(L, jacobi, ell=9, rule=5, work_size=1)[1]
    assert "unknown stop rule 5" in _call(L, jacobi, rule=5, work_size=1)[1]
    assert "the work vector holds 1 entries" in _call(L, jacobi, work_size=1, dinv=TINY)[1]


def test_an_odd_row_count_rounds_the_slices_up_to_even(hiplib):
    """9 rows: slices 10 apart, so l = 2 needs 40 entries and 36 are refused."""
    L = hiplib
    head = _VectorHead(None, 39, -1, b"")
    nine = _VectorHead(None, 9, -1, b"")
    v9 = C.addressof(nine)
    L.MgcgClearLastError()
    st = L.SolveBicgstabL(H, H, None, *([v9] * 8), C.addressof(head), 2, 25, 9, *STOP, _lib.RULE_CSHARP, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    assert st == _lib.ERROR and "holds 39 entries, ell = 2 needs 40 (4 slices of 10: the matrix has 9 rows)" in msg, msg
