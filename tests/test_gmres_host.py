"""Restarted GMRES(m) on the host side (no GPU needed): the yardstick of tests/test_gpu_gmres.py lives here and is checked against the true
residual, against ``bicgstab_oracle`` on the two systems that loop cannot solve, and on the corner cases of the method; the library exports
the two entry points and refuses bad arguments before it asks for a device.

``gmres_oracle`` is the loop of include/MgcgGpu.h (SolveGmres / SolveGmresJacobi) in np.float64, operation by operation: every product goes
into a named array or scalar before the add that follows it, a matrix row is summed serially in stored order from +0.0 (``row_sums``), the
orthogonalisation is classical Gram-Schmidt applied ``orth`` times with the subtractions one column at a time in ascending order, the
rotations and the back substitution are evaluated in the header's order, x is updated in groups of eight columns, and every sum is a serial
left-to-right sum (``serial_sum``).  Under dot_order = 1 the HIP loop must EQUAL it.

Systems: every case listed in CASES met 1.001 x the stop level with serial sums, so none was replaced.  The non-increasing trace holds for
orth = 2 AND for orth = 1 on every case (test_the_trace_never_increases reports both)."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_bicgstab_host import _classical_cg_solution, bicgstab_oracle, nonsymmetric_tridiagonal, numpy_true_residual, small
from tests.test_bicgstabl_host import MATRICES as L_MATRICES
from tests.test_mixed_host import row_sums, serial_sum
from tests.test_sreduce_host import diagonal_of, stop_decision, with_b
from tests.test_variant_refusals_host import EIGHT, H, OUT3, SHORT, STOP, TINY, VEC, _VectorHead

DBL_BIG = 1.79e308
MAX_M = 32
GROUP = 8                                                                          # columns per update / x-update launch


# --------------------------------------------------------------------------- the yardstick
def gmres_oracle(s, m, orth, dinv=None, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, x0=None, total=serial_sum):
    """A x = s.b from s.x (x0) by GMRES(m), right-preconditioned with diag(1 / dinv) when dinv is given; ``orth`` Gram-Schmidt passes per
    step.  total(terms): the sum of the terms (default: serial, left to right).  Returns x, r (= b - A x, the closing product), iteration
    (Arnoldi steps), residual, true_residual, status, trace; and ``gap``: the largest |restart's explicit || r || - rotated estimate|."""
    assert 1 <= m <= MAX_M and orth in (1, 2)
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    n = s.Count
    f = np.float64

    def sums(terms):
        return f(total(terms))

    def dots(V, w):                                                               # V_i.w for every row of V
        if total is serial_sum:
            return np.add.accumulate(V * w, axis=1)[:, -1] if n else np.zeros(len(V))
        return np.array([total(row) for row in V * w])

    def finite(v):
        return bool(abs(v) <= DBL_BIG)

    def hat(v):
        return v if dinv is None else dinv * v

    gap = [0.0]

    def closing(x, it, res, status, trace):
        r = b - row_sums(e, c, ro, x)
        with np.errstate(all="ignore"):
            true = float(np.sqrt(sums(r * r)))
        return dict(x=x, r=r, iteration=it, residual=res, true_residual=true, status=status, trace=np.array(trace), gap=gap[0])

    with np.errstate(all="ignore"):
        x = np.zeros(n) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
        r = b - row_sums(e, c, ro, x)
        beta2 = rr0 = sums(r * r)
        res = float(np.sqrt(rr0))
        shown = float(np.sqrt(rr0 / rr0)) if rule == _lib.RULE_VIENNACL else res
        trace = [shown]
        if not (0.0 < rr0 <= DBL_BIG):
            return closing(x, 0, res, _lib.NONFINITE, trace)
        k = 0
        V = np.empty((m + 1, n))
        Rm = np.zeros((m, m))
        while True:                                                               # one cycle
            beta = np.sqrt(beta2)
            V[0] = r / beta
            g = [beta]
            cs, sn = [], []
            cols, ended = 0, None
            for j in range(m):
                w = row_sums(e, c, ro, hat(V[j]))
                h = None
                for p in range(orth):
                    hp = dots(V[: j + 1], w)
                    terms = hp[:, None] * V[: j + 1]                              # h'_i v_i, each into an array of its own
                    w = np.subtract.accumulate(np.vstack([w[None, :], terms]), axis=0)[-1]   # ((w - t_0) - t_1) - ...
                    h = hp.copy() if p == 0 else h + hp
                hn2 = sums(w * w)
                hn = np.sqrt(hn2)
                for i in range(j):                                                # the stored rotations
                    t1 = cs[i] * h[i]
                    t2 = sn[i] * h[i + 1]
                    t3 = sn[i] * h[i]
                    t4 = cs[i] * h[i + 1]
                    h[i] = t1 + t2
                    h[i + 1] = t4 - t3
                p1 = h[j] * h[j]
                p2 = hn * hn
                d = np.sqrt(p1 + p2)
                if not finite(hn2) or d == 0.0 or not finite(d):                  # no next direction, and no column: the last judged figure again
                    trace.append(shown)
                    ended = (k + 1, res, _lib.NONFINITE)
                    break
                cj = h[j] / d
                sj = hn / d
                ms = -sj
                gn = ms * g[j]
                g[j] = cj * g[j]
                g.append(gn)
                cs.append(cj)
                sn.append(sj)
                Rm[: j, j] = h[: j]
                Rm[j, j] = d
                cols = j + 1
                gg = gn * gn
                res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, gg, rr0)
                if hn2 == 0.0:                                                    # the Krylov space is exhausted: x will be exact
                    stop, status = True, _lib.OK
                trace.append(shown)
                k += 1
                if stop:
                    ended = (k, res, status)
                    break
                V[j + 1] = w / hn
            # the close: y = R^-1 g over the completed columns, x += hat(sum y_i v_i) in groups of eight columns
            y = np.zeros(cols)
            for i in range(cols - 1, -1, -1):
                acc = g[i]
                for q in range(i + 1, cols):
                    t = Rm[i, q] * y[q]
                    acc = acc - t
                y[i] = acc / Rm[i, i]
            for g0 in range(0, cols, GROUP):
                g1 = min(g0 + GROUP, cols)
                terms = y[g0:g1, None] * V[g0:g1]
                acc = np.add.accumulate(np.vstack([np.zeros((1, n)), terms]), axis=0)[-1]
                x = x + hat(acc)
            if ended is not None:
                return closing(x, ended[0], ended[1], ended[2], trace)
            r = b - row_sums(e, c, ro, x)                                         # the restart
            beta2 = sums(r * r)
            if rule != _lib.RULE_VIENNACL:
                gap[0] = max(gap[0], abs(float(np.sqrt(beta2)) - res))
            if beta2 == 0.0:
                return closing(x, k, 0.0, _lib.OK, trace)
            if not finite(beta2):
                return closing(x, k, res, _lib.NONFINITE, trace)


# --------------------------------------------------------------------------- the systems
SEED = 20261019
MATRICES = dict(L_MATRICES)
MATRICES["tridiagonal300"] = lambda: nonsymmetric_tridiagonal(300)
MATRICES["tridiagonal300_19"] = lambda: nonsymmetric_tridiagonal(300, -1.9, 2.0, -0.1)
CONVERGENCE = ["tridiagonal300", "convdiff16", "convdiff32x32_5", "convdiff15x15x3", "upwind16", "random_nonsymmetric4097", "poisson16"]
MS = [1, 2, 8, 9, 17, 32]
ORTHS = [1, 2]
CASES = [(name, rhs, m) for name in CONVERGENCE for rhs in ("ones", "randn") for m in MS]
MAX_IT = 20000
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


def level_of(s, rel=1e-8):
    return rel * float(np.linalg.norm(s.b))


def run(name, rhs, m, orth, jacobi, rel=1e-8, max_it=MAX_IT):
    """The yardstick's run to a relative ``rel`` with serial sums, computed once and shared (nothing changes it)."""
    key = (name, rhs, m, orth, jacobi, rel, max_it)
    if key not in _runs:
        s, dinv = system(name, rhs)
        _runs[key] = gmres_oracle(s, m, orth, dinv if jacobi else None, _lib.RULE_CSHARP, level_of(s, rel), max_it=max_it)
    return _runs[key]


def never_increases(trace):
    """Every entry is at most one ulp above the one before."""
    t = np.asarray(trace)
    return bool((t[1:] <= np.nextafter(t[:-1], np.inf)).all())


# --------------------------------------------------------------------------- convergence
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("name,rhs,m", CASES)
def test_the_true_residual_is_within_the_stop_level(name, rhs, m, orth, jacobi):
    s, _ = system(name, rhs)
    level = level_of(s)
    o = run(name, rhs, m, orth, jacobi)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs} m={m} orth={orth} jacobi={jacobi}: {o['iteration']} steps, estimate {o['residual']:.3e}, true {true:.3e} = {true / level:.4f} x "
          f"the stop level, |true - estimate| = {abs(true - o['residual']) / level:.2e} x the level, restart gap {o['gap'] / level:.2e} x the level")
    assert o["status"] == _lib.OK
    assert o["residual"] < level
    assert true <= 1.001 * level
    assert abs(true - o["residual"]) <= 1e-4 * level
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name,rhs,m", CASES)
def test_the_trace_never_increases(name, rhs, m, jacobi):
    """Asserted with orth = 2; the same check with orth = 1 is reported."""
    one = never_increases(run(name, rhs, m, 1, jacobi)["trace"])
    print(f"{name} {rhs} m={m} jacobi={jacobi}: orth = 1 trace non-increasing: {one}")
    assert never_increases(run(name, rhs, m, 2, jacobi)["trace"])


# --------------------------------------------------------------------------- the capability
CAPS = {"convdiff32x32_20": 750, "tridiagonal300_19": 1500}


def test_gmres_converges_where_bicgstab_breaks_down():
    s, _ = system("convdiff32x32_20", "ones")
    level = level_of(s)
    old = bicgstab_oracle(s, None, _lib.RULE_CSHARP, level, max_it=3000)
    print(f"bicgstab_oracle: status {old['status']} at body {old['iteration']}")
    assert old["status"] == _lib.NONFINITE
    for m in (20, 5):
        o = run("convdiff32x32_20", "ones", m, 2, False, max_it=CAPS["convdiff32x32_20"])
        true = numpy_true_residual(s, o["x"])
        print(f"GMRES({m}): {o['iteration']} steps, true residual {true / level:.4f} x the level")
        assert o["status"] == _lib.OK and true <= 1.001 * level


def test_gmres_does_not_drift_where_bicgstab_does():
    s, _ = system("tridiagonal300_19", "ones")
    level = level_of(s)
    old = bicgstab_oracle(s, None, _lib.RULE_CSHARP, level, max_it=3000)
    true_old = numpy_true_residual(s, old["x"])
    print(f"bicgstab_oracle: status {old['status']}, recurrence {old['residual']:.3e}, true residual {true_old:.3e}")
    assert not (true_old <= 1e6 * max(old["residual"], level))                    # far above its recurrence's figure, or not a number
    o = run("tridiagonal300_19", "ones", 20, 2, False, max_it=CAPS["tridiagonal300_19"])
    true = numpy_true_residual(s, o["x"])
    print(f"GMRES(20): {o['iteration']} steps, true residual {true / level:.4f} x the level")
    assert o["status"] == _lib.OK and true <= 1.001 * level


# --------------------------------------------------------------------------- rules, start, minimum, cap
@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule):
    s, _ = system("convdiff16", "randn")
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else level_of(s)
    o = gmres_oracle(start, 9, 2, None, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 10
    zero = gmres_oracle(s, 9, 2, None, rule, tol, max_it=MAX_IT)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert (o["iteration"] == zero["iteration"] and np.array_equal(o["x"], zero["x"])) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2] and zero["trace"][0] == 1.0
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]
        assert numpy_true_residual(s, o["x"]) <= 1.001 * tol


def test_the_minimum_is_kept_five_steps_beyond_convergence():
    s, _ = system("convdiff16", "randn")
    tol = 1e-6 * float(np.linalg.norm(s.b))
    free = gmres_oracle(s, 9, 2, None, tol=tol, max_it=400)
    held = gmres_oracle(s, 9, 2, None, tol=tol, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    assert np.array_equal(held["trace"][: free["iteration"] + 1], free["trace"])
    assert numpy_true_residual(s, held["x"]) <= 1.001 * tol


@pytest.mark.parametrize("m,cap", [(9, 12), (9, 8), (4, 3)])
def test_the_cap_ends_the_loop_with_x_closed_in_mid_cycle(m, cap):
    """iteration = cap + 1, and x is what the close made of the columns the cut cycle completed: the estimate and the true residual agree."""
    s, _ = system("convdiff16", "randn")
    o = gmres_oracle(s, m, 2, None, tol=0.0, max_it=cap)
    assert o["status"] == _lib.MAXIT_EXCEEDED and o["iteration"] == cap + 1 and len(o["trace"]) == cap + 2
    true = numpy_true_residual(s, o["x"])
    assert abs(true - o["residual"]) <= 1e-10 * true


def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0():
    s = nonsymmetric_tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = gmres_oracle(with_b(s, np.zeros(50), "b0"), 9, 2, None, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


# --------------------------------------------------------------------------- tiny systems and the two no-next-direction branches
def test_one_row_takes_one_step_with_hn_zero_and_x_exact():
    s = nonsymmetric_tridiagonal(1)
    for orth in ORTHS:
        o = gmres_oracle(s, 32, orth, None, tol=level_of(s), min_it=7)            # whatever minIteration says
        assert o["status"] == _lib.OK and o["iteration"] == 1 and o["residual"] == 0.0 and o["true_residual"] == 0.0
        assert np.array_equal(o["x"], [1.0]) and list(o["trace"]) == [2.0, 0.0]


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("n,m", [(2, 32), (3, 32), (7, 32), (7, 4)])
def test_tiny_systems_end_cleanly(n, m, orth, jacobi):
    s = nonsymmetric_tridiagonal(n)
    level = level_of(s)
    o = gmres_oracle(s, m, orth, 1.0 / diagonal_of(s) if jacobi else None, tol=level)
    true = numpy_true_residual(s, o["x"])
    print(f"n = {n} m = {m} orth = {orth} jacobi={jacobi}: status {o['status']} after {o['iteration']} steps, true residual {true:.3e}")
    assert o["status"] == _lib.OK and true <= 1.001 * level
    if m >= n:
        assert o["iteration"] <= n


def singular2():
    """[[1, 0], [0, 0]] with the zero diagonal stored, b = (0, 1): v_0 = b, w = A v_0 = 0, h = 0, hn = 0 and d = 0 in step 0, all exact."""
    return small([[1.0, 0.0], [0.0, 0.0]], [0.0, 1.0], "singular2", x=[0.0, 0.0])


@pytest.mark.parametrize("orth", ORTHS)
def test_the_singular_branch_gives_nonfinite_at_step_1_and_the_callers_x_back(orth):
    s = singular2()
    o = gmres_oracle(s, 9, orth, None, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], [0.0, 0.0])
    assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0


def test_the_exhausted_branch_in_the_second_step():
    """[[1, 1], [0, 1]], b = (0, 1): step 0 has h = 1 and hn = 1, step 1 has w = A (1, 0) = (1, 0), h' = (0, 1) and hn = 0 exactly."""
    s = small([[1.0, 1.0], [0.0, 1.0]], [0.0, 1.0], "exhausted2", x=[0.0, 0.0])
    o = gmres_oracle(s, 9, 2, None, tol=0.0, min_it=5)
    assert o["status"] == _lib.OK and o["iteration"] == 2 and o["residual"] == 0.0
    assert np.allclose(o["x"], [-1.0, 1.0], rtol=1e-15, atol=1e-15)


# --------------------------------------------------------------------------- equivalences
@pytest.mark.parametrize("orth", ORTHS)
def test_a_uniform_diagonal_of_4_gives_the_plain_loops_bits(orth):
    s, dinv = system("convdiff32x32_5", "randn")
    assert (dinv == 0.25).all()
    for m in (8, 9):
        plain, jacobi = run("convdiff32x32_5", "randn", m, orth, False), run("convdiff32x32_5", "randn", m, orth, True)
        assert jacobi["iteration"] == plain["iteration"] and np.array_equal(jacobi["x"], plain["x"]) and np.array_equal(jacobi["trace"], plain["trace"])


def test_poisson_agrees_with_classical_cg():
    s, _ = system("poisson16", "randn")
    ref = _classical_cg_solution(s, 200)
    assert numpy_true_residual(s, ref) <= 1e-10 * float(np.linalg.norm(s.b))
    for m in (9, 32):
        x = run("poisson16", "randn", m, 2, False)["x"]
        assert np.max(np.abs(x - ref)) <= 1e-6 * np.max(np.abs(ref))


# --------------------------------------------------------------------------- the library's host side
EXPORTS = ("SolveGmres", "SolveGmresJacobi")


def test_both_symbols_are_exported_and_bound(hiplib):
    for name in EXPORTS:
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["SolveGmres"][1] == _lib.SIGNATURES["SolveBicgstabL"][1][:12] + [C.c_int] + _lib.SIGNATURES["SolveBicgstabL"][1][12:]


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import bicgstab, gmres

    assert "GMRES" in conjugategradient_amd.__doc__ and "gmres" in conjugategradient_amd.__all__ and "GMRES" in gmres.__doc__
    assert issubclass(gmres.GeneralizedMinimalResidualGpu, bicgstab.BiConjugateGradientStabGpu)
    assert issubclass(gmres.GeneralizedMinimalResidualJacobiGpu, gmres.GeneralizedMinimalResidualGpu)
    for cls in (gmres.GeneralizedMinimalResidualGpu, gmres.GeneralizedMinimalResidualJacobiGpu):
        cg = cls.__new__(cls)
        cg._ready = False
        with pytest.raises(_lib.MgcgError, match="Initialize"):
            cg.Solve()
        with pytest.raises(ValueError, match="max-norm"):
            cls(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
        with pytest.raises(ValueError, match="max-norm"):
            cls(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL, m=4, orth=1)


def _call(L, jacobi, blas=H, sparse=H, work=None, dinv=VEC, m=4, orth=2, rule=_lib.RULE_CSHARP, work_size=None):
    """One call with zeroed handles and vector heads of 10 entries: a refused call looks at nothing else.  (status, message)"""
    head = _VectorHead(None, (400 if work_size is None else work_size), -1, b"")
    if work is None:
        work = C.addressof(head)
    elif work == "null":
        work = None
    L.MgcgClearLastError()
    fn = L.SolveGmresJacobi if jacobi else L.SolveGmres
    st = fn(blas, sparse, None, *EIGHT, work, *((dinv,) if jacobi else ()), m, orth, 28, 10, *STOP, rule, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    return st, msg


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib, jacobi):
    L = hiplib
    who = "SolveGmresJacobi" if jacobi else "SolveGmres"
    for kw in [dict(blas=None), dict(sparse=None), dict(work="null")] + ([dict(dinv=None)] if jacobi else []):
        st, msg = _call(L, jacobi, **kw)
        assert st == _lib.ERROR and msg == f"{who}: null handle", (kw, msg)
    for m in (0, 33, -1, 100):
        st, msg = _call(L, jacobi, m=m)
        assert st == _lib.ERROR and msg == f"{who}: m = {m}, must be 1 .. 32", msg
    for orth in (0, 3, -1):
        st, msg = _call(L, jacobi, orth=orth)
        assert st == _lib.ERROR and msg == f"{who}: orth = {orth}, must be 1 or 2", msg
    st, msg = _call(L, jacobi, rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "MGCG_RULE_HANDMADECL" in msg and msg.startswith(f"{who}:")
    for rule in (-1, 5):
        st, msg = _call(L, jacobi, rule=rule)
        assert st == _lib.ERROR and msg == f"{who}: unknown stop rule {rule}"
    # 10 rows: slices of 10 entries, m + 1 of them and one more with the diagonal
    for m in (1, 8, 9, 32):
        slices = m + 1 + (1 if jacobi else 0)
        need = slices * 10
        st, msg = _call(L, jacobi, m=m, work_size=need - 1)
        assert st == _lib.ERROR and f"the work vector holds {need - 1} entries, m = {m} needs {need} ({slices} slices of 10: the matrix has 10 rows)" in msg, msg
    if jacobi:
        st, msg = _call(L, jacobi, dinv=SHORT)
        assert st == _lib.ERROR and "the dinv vector holds 9 entries" in msg
    # m is looked at before orth, orth before the rule, the rule before the work vector, the work vector before dinv
    assert "m = 40" in _call(L, jacobi, m=40, orth=7, rule=5, work_size=1)[1]
    assert "orth = 7" in _call(L, jacobi, orth=7, rule=5, work_size=1)[1]
    assert "unknown stop rule 5" in _call(L, jacobi, rule=5, work_size=1)[1]
    assert "the work vector holds 1 entries" in _call(L, jacobi, work_size=1, dinv=TINY)[1]


def test_an_odd_row_count_rounds_the_slices_up_to_even(hiplib):
    """9 rows: slices 10 apart, so m = 3 needs 40 entries and 39 are refused."""
    L = hiplib
    head = _VectorHead(None, 39, -1, b"")
    nine = _VectorHead(None, 9, -1, b"")
    v9 = C.addressof(nine)
    L.MgcgClearLastError()
    st = L.SolveGmres(H, H, None, *([v9] * 8), C.addressof(head), 3, 2, 25, 9, *STOP, _lib.RULE_CSHARP, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    assert st == _lib.ERROR and "holds 39 entries, m = 3 needs 40 (4 slices of 10: the matrix has 9 rows)" in msg, msg
