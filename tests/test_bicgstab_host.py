"""BiCGStab on the host side (no GPU needed): the yardstick of tests/test_gpu_bicgstab.py lives here and is checked against the true
residual, against classical CG on symmetric matrices and on the corner cases of the method; the library exports the four entry points and
refuses bad arguments before it asks for a device.

``bicgstab_oracle`` is the loop of include/MgcgGpu.h (SolveBicgstab / SolveBicgstabJacobi) in np.float64: every product goes into a named
array or scalar before the add that follows it, a matrix row is summed serially in stored order from +0.0 (``row_sums``), the scalars are
evaluated in the header's order, and every sum is a serial left-to-right sum (``serial_sum``), cut at ``parts`` and added in rank order.
Under dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums
from tests.test_sreduce_host import classical_cg_iteration, diagonal_of, serial_sum, stop_decision, with_b

DBL_BIG = 1.79e308


# --------------------------------------------------------------------------- the yardstick
def bicgstab_oracle(s, dinv=None, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, parts=None, x0=None, total=serial_sum):
    """A x = s.b from s.x (x0), right-preconditioned with diag(1 / dinv) when dinv is given.  total(terms): the sum of one rank's terms
    (default: serial, left to right)."""
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

    def closing(x, it, res, status, trace):
        r = b - row_sums(e, c, ro, x)
        with np.errstate(all="ignore"):
            true = float(np.sqrt(sums(r * r)))
        return dict(x=x, r=r, iteration=it, residual=res, true_residual=true, status=status, trace=np.array(trace))

    with np.errstate(all="ignore"):
        x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
        r = b - row_sums(e, c, ro, x)
        rhat = r.copy()
        p = r.copy()
        phat = hat(p)
        rho = rr0 = sums(r * r)
        res = float(np.sqrt(rr0))
        shown = float(np.sqrt(rr0 / rr0)) if rule == _lib.RULE_VIENNACL else res
        trace = [shown]
        if not (0.0 < rr0 <= DBL_BIG):
            return closing(x, 0, res, _lib.NONFINITE, trace)
        k = 0
        while True:
            v = row_sums(e, c, ro, phat)
            sigma = sums(rhat * v)
            alpha = rho / sigma
            if sigma == 0.0 or not finite(sigma) or not finite(alpha):      # breakdown, before this body's updates: the last judged figure again
                trace.append(shown)
                return closing(x, k + 1, res, _lib.NONFINITE, trace)
            av = alpha * v
            sv = r - av
            shat = hat(sv)
            t = row_sums(e, c, ro, shat)
            theta = sums(sv * t)
            tau = sums(t * t)
            omega = f(0.0) if tau == 0.0 else theta / tau
            if not finite(omega):
                trace.append(shown)
                return closing(x, k + 1, res, _lib.NONFINITE, trace)
            ap = alpha * phat
            x1 = x + ap
            os_ = omega * shat
            x = x1 + os_
            ot = omega * t
            r = sv - ot
            rr = sums(r * r)
            rhon = sums(rhat * r)
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, rr, rr0)
            trace.append(shown)
            if not stop and (omega == 0.0 or rhon == 0.0 or not finite(rhon)):    # x IS this body's iterate
                stop, status = True, _lib.NONFINITE
            if stop:
                return closing(x, k + 1, res, status, trace)
            q1, q2 = rhon / rho, alpha / omega
            beta = q1 * q2
            ov = omega * v
            pm = p - ov
            bp = beta * pm
            p = r + bp
            phat = hat(p)
            rho = rhon
            k += 1


# --------------------------------------------------------------------------- what it is measured against
def _product(s, v):
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * v[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


def numpy_true_residual(s, x):
    """|| b - A x ||_2 with numpy's own sums: independent of the yardstick's arithmetic."""
    return float(np.linalg.norm(s.b - _product(s, x)))


def small(rows, b, name, x=None):
    """A dense list of rows as CSR (every entry stored)."""
    a = np.array(rows, dtype=np.float64)
    n = a.shape[0]
    return problems.LinearSystem(a.ravel().copy(), np.tile(np.arange(n, dtype=np.int32), n), np.arange(0, n * n + 1, n, dtype=np.int32),
                                 np.zeros(n) if x is None else np.array(x, dtype=np.float64), np.array(b, dtype=np.float64), name)


def nonsymmetric_tridiagonal(n, lower=-1.5, diag=2.0, upper=-0.5):
    """(lower, diag, upper) on the three diagonals, columns ascending; b = A.1, x0 = 0."""
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    vals = np.tile(np.array([lower, diag, upper]), (n, 1))
    keep = (cols >= 0) & (cols < n)
    ro = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    s = problems.LinearSystem(vals[keep], cols[keep].astype(np.int32), ro, np.zeros(n), np.zeros(n), f"nonsymmetric_tridiagonal{n}")
    return with_b(s, _product(s, np.ones(n)), s.name)


def sigma_zero2():
    """[[1, -3], [1, 1]], b = (1, 1): v = A b = (-2, 2) and sigma = rhat.v = 0 in body 0, exactly."""
    return small([[1.0, -3.0], [1.0, 1.0]], [1.0, 1.0], "sigma_zero2", x=[0.0, 0.0])


def rho_zero2():
    """[[2, 0], [2, 4]], b = (1, 1): every operation of body 0 is exact -- alpha = 1/4, s = (1/2, -1/2) is an eigenvector, t = 2 s,
    omega = 1/2, r = 0 and rhon = 0 -- and x = (1/2, 0) solves the system.  With tolerance 0 no rule stops, so the rhon == 0 branch does."""
    return small([[2.0, 0.0], [2.0, 4.0]], [1.0, 1.0], "rho_zero2", x=[0.0, 0.0])


SEED = 20261019
MATRICES = {
    "tridiagonal300": lambda: nonsymmetric_tridiagonal(300),
    "convdiff16": lambda: problems.convection_diffusion(16, 16, 16, (0.5, 0.25, 0.0)),
    "convdiff16strong": lambda: problems.convection_diffusion(16, 16, 16, (0.9, 0.9, 0.9)),
    "upwind16": lambda: problems.convection_diffusion(16, 16, 16, (2.0, 1.0, 0.5), upwind=True),
    "convdiff32x32": lambda: problems.convection_diffusion(32, 32, 1, (0.5, 0.25)),
    "random_nonsymmetric5000": lambda: problems.random_nonsymmetric(5000, 9, SEED),
    "poisson16": lambda: problems.poisson(16, 16, 16),
}
CASES = [(m, rhs) for m in MATRICES for rhs in ("ones", "randn")]
SYMMETRIC = ["poisson16"]
MAX_IT = 3000
ORDERS = {"serial": serial_sum, "pairwise": lambda terms: float(np.sum(terms)) if len(terms) else 0.0, "exact": lambda terms: math.fsum(terms)}
_systems, _runs = {}, {}


def system(name, rhs="ones"):
    """(system, dinv): the matrix with b = A.1 ("ones") or an N(0,1) b of fixed seed ("randn"), and 1 / diag(A)."""
    key = (name, rhs)
    if key not in _systems:
        s = MATRICES[name]()
        b = _product(s, np.ones(s.Count)) if rhs == "ones" else np.random.default_rng(SEED).standard_normal(s.Count)
        s = with_b(s, b, f"{name}-{rhs}")
        _systems[key] = (s, 1.0 / diagonal_of(s))
    return _systems[key]


def run(name, rhs, jacobi, order="serial", rel=1e-8):
    """The yardstick's run to a relative ``rel``, computed once and shared (nothing changes it)."""
    key = (name, rhs, jacobi, order, rel)
    if key not in _runs:
        s, dinv = system(name, rhs)
        _runs[key] = bicgstab_oracle(s, dinv if jacobi else None, _lib.RULE_CSHARP, rel * float(np.linalg.norm(s.b)), max_it=MAX_IT, total=ORDERS[order])
    return _runs[key]


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name,rhs", CASES)
def test_the_true_residual_is_within_the_stop_level(name, rhs, jacobi, order):
    """The condition on the chosen inputs that makes the factor 1.001 of the GPU tests safe: the recurrence's residual and the true one
    agree to 1e-4 of the stop level (fifty times the 2e-6 observed)."""
    s, _ = system(name, rhs)
    level = 1e-8 * float(np.linalg.norm(s.b))
    o = run(name, rhs, jacobi, order)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs} jacobi={jacobi} {order}: {o['iteration']} bodies, recurrence {o['residual']:.3e}, true {true:.3e} = {true / level:.4f} x the stop level, "
          f"|true - recurrence| = {abs(true - o['residual']) / level:.2e} x the level")
    assert o["status"] == _lib.OK
    assert o["residual"] < level
    assert true <= 1.001 * level
    assert abs(true - o["residual"]) <= 1e-4 * level
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    if order == "serial":
        assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


def test_jacobi_needs_fewer_bodies_on_an_uneven_diagonal_and_the_same_on_a_uniform_one():
    for rhs in ("ones", "randn"):
        plain, jacobi = run("random_nonsymmetric5000", rhs, False), run("random_nonsymmetric5000", rhs, True)
        print(f"random_nonsymmetric5000 {rhs}: plain {plain['iteration']} bodies, Jacobi {jacobi['iteration']}")
        assert jacobi["iteration"] < plain["iteration"]
    # a uniform diagonal d: M = d I only scales phat and shat, and alpha and omega by 1 / d in return; with d a power of two nothing else moves
    s, dinv = system("convdiff32x32", "randn")
    assert (dinv == 0.25).all()
    plain, jacobi = run("convdiff32x32", "randn", False), run("convdiff32x32", "randn", True)
    assert jacobi["iteration"] == plain["iteration"] and np.array_equal(jacobi["x"], plain["x"])
    for name in ("convdiff16", "poisson16"):                                       # d = 6: the same up to rounding
        assert run(name, "randn", True)["iteration"] == run(name, "randn", False)["iteration"]


def _classical_cg_solution(s, bodies):
    """x after `bodies` bodies of textbook float64 CG from x = 0 (the loop of classical_cg_iteration)."""
    b = np.asarray(s.b, dtype=np.float64)
    x, r = np.zeros(s.Count), b.copy()
    p, rr = r.copy(), float(r @ r)
    for _ in range(bodies):
        Ap = _product(s, p)
        alpha = rr / float(p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("rhs", ["ones", "randn"])
@pytest.mark.parametrize("name", SYMMETRIC)
def test_symmetric_systems_agree_with_classical_cg(name, rhs, jacobi):
    s, _ = system(name, rhs)
    goal = 1e-8 * float(np.linalg.norm(s.b))
    x_cg = _classical_cg_solution(s, classical_cg_iteration(s, goal) + 1)
    o = run(name, rhs, jacobi)
    distance = float(np.linalg.norm(o["x"] - x_cg) / np.linalg.norm(x_cg))
    print(f"{name} {rhs} jacobi={jacobi}: BiCGStab {o['iteration']} bodies, distance to classical CG's x {distance:.3e}")
    assert o["status"] == _lib.OK and distance <= 1e-6


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule):
    s, _ = system("convdiff16", "randn")
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else 1e-8 * float(np.linalg.norm(s.b))
    o = bicgstab_oracle(start, None, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 10
    zero = bicgstab_oracle(s, None, rule, tol, max_it=MAX_IT)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert (o["iteration"] == zero["iteration"] and np.array_equal(o["x"], zero["x"])) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2] and zero["trace"][0] == 1.0
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]


def test_the_iteration_cap_and_the_minimum_are_kept():
    s, _ = system("convdiff16", "randn")
    capped = bicgstab_oracle(s, None, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    tol = 1e-2 * float(np.linalg.norm(s.b))
    free = bicgstab_oracle(s, None, tol=tol, max_it=400)
    held = bicgstab_oracle(s, None, tol=tol, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_tiny_systems_finish_in_at_most_n_bodies(n, jacobi):
    s = nonsymmetric_tridiagonal(n)
    o = bicgstab_oracle(s, 1.0 / diagonal_of(s) if jacobi else None, tol=1e-8 * float(np.linalg.norm(s.b)))
    print(f"n = {n} jacobi={jacobi}: {o['iteration']} bodies, residual {o['residual']:.3e}")
    assert o["status"] == _lib.OK and 1 <= o["iteration"] <= n
    assert np.allclose(o["x"], np.ones(n), rtol=1e-7, atol=0)


def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0():
    s = nonsymmetric_tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = bicgstab_oracle(with_b(s, np.zeros(50), "b0"), None, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


def test_sigma_zero_gives_nonfinite_and_the_callers_x_back():
    s = sigma_zero2()
    s.x[:] = 0.0
    o = bicgstab_oracle(s, None, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], s.x)
    root2 = math.sqrt(2.0)
    assert list(o["trace"]) == [root2, root2] and o["residual"] == root2 and o["true_residual"] == root2
    # from another start the same matrix is solved: it is not singular
    ok = bicgstab_oracle(s, None, tol=1e-12, x0=[0.0, 1.0])
    assert ok["status"] == _lib.OK and numpy_true_residual(s, ok["x"]) < 1e-12


def test_rhon_zero_gives_nonfinite_with_this_bodys_iterate():
    s = rho_zero2()
    o = bicgstab_oracle(s, None, tol=0.0)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1
    assert np.array_equal(o["x"], [0.5, 0.0]) and o["residual"] == 0.0 and o["true_residual"] == 0.0
    assert list(o["trace"]) == [math.sqrt(2.0), 0.0]
    # with a tolerance the same body is a convergence
    ok = bicgstab_oracle(s, None, tol=1e-12)
    assert ok["status"] == _lib.OK and ok["iteration"] == 1 and np.array_equal(ok["x"], [0.5, 0.0])


def test_sums_are_cut_at_the_ranks_and_added_in_rank_order():
    s, dinv = system("random_nonsymmetric5000", "randn")
    tol = 1e-8 * float(np.linalg.norm(s.b))
    one = run("random_nonsymmetric5000", "randn", False)
    cut = bicgstab_oracle(s, None, tol=tol, max_it=MAX_IT, parts=problems.partition_offsets(s.Count, 3))
    # another summation order, the same method
    assert not np.array_equal(one["x"], cut["x"]) and cut["status"] == _lib.OK
    assert abs(one["iteration"] - cut["iteration"]) <= 2
    assert numpy_true_residual(s, cut["x"]) <= 1.001 * tol
    empty = bicgstab_oracle(s, None, tol=tol, max_it=MAX_IT, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- the library's host side
EXPORTS = ("SolveBicgstab", "SolveBicgstabJacobi", "SolveBicgstabParallel", "SolveBicgstabJacobiParallel")


def test_the_four_symbols_are_exported_and_bound(hiplib):
    for name in EXPORTS:
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import bicgstab, parallel

    assert "bicgstab" in conjugategradient_amd.__all__ and "``bicgstab``" in conjugategradient_amd.__doc__
    assert issubclass(bicgstab.BiConjugateGradientStabGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    assert issubclass(bicgstab.BiConjugateGradientStabJacobiGpu, bicgstab.BiConjugateGradientStabGpu)
    assert callable(parallel.ConjugateGradientRankGpu.SolveBicgstab) and callable(parallel.ConjugateGradientRankGpu.SolveBicgstabJacobi)
    for cls in (bicgstab.BiConjugateGradientStabGpu, bicgstab.BiConjugateGradientStabJacobiGpu):
        cg = cls.__new__(cls)
        cg._ready = False
        with pytest.raises(_lib.MgcgError, match="Initialize"):
            cg.Solve()
        with pytest.raises(ValueError, match="max-norm"):
            cls(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)


def test_the_builders_make_what_they_say():
    p = problems.poisson(5, 4, 3)
    c0 = problems.convection_diffusion(5, 4, 3)
    assert np.array_equal(c0.Elements, p.Elements) and np.array_equal(c0.ColumnIndeces, p.ColumnIndeces) and np.array_equal(c0.RowOffsets, p.RowOffsets)
    a = problems.convection_diffusion(5, 4, 1, (0.5, 0.25)).to_scipy().toarray()
    assert a[6, 6] == 4.0 and a[6, 5] == -1.5 and a[6, 7] == -0.5 and a[6, 1] == -1.25 and a[6, 11] == -0.75
    u = problems.convection_diffusion(5, 4, 3, (2.0, 1.0, 0.5), upwind=True).to_scipy().toarray()
    row = 20 + 5 + 1
    assert u[row, row] == 13.0 and u[row, row - 1] == -5.0 and u[row, row + 1] == -1.0 and u[row, row - 5] == -3.0 and u[row, row + 5] == -1.0
    assert u[row, row - 20] == -2.0 and u[row, row + 20] == -1.0
    r = problems.random_nonsymmetric(400, 9, 7)
    a = r.to_scipy().toarray()
    off = np.abs(a).sum(axis=1) - np.abs(np.diag(a))
    assert (np.diag(a) >= off + 0.5).all() and (np.diag(a) <= off + 50.0).all() and not np.array_equal(a, a.T)
    assert int(np.diff(r.RowOffsets).max()) <= 9 and np.array_equal(r.b, r.to_scipy() @ np.ones(400))
    same = problems.random_nonsymmetric(400, 9, 7)
    assert np.array_equal(same.Elements, r.Elements) and np.array_equal(same.ColumnIndeces, r.ColumnIndeces)


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    handle = C.create_string_buffer(4096)                  # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    big, small_ = _VectorHead(None, 10, -1, b""), _VectorHead(None, 9, -1, b"")
    vec, short = C.addressof(big), C.addressof(small_)

    def call(jacobi, blas=h, sparse=h, v=vec, s=vec, t=vec, rhat=vec, dinv=vec, rule=_lib.RULE_CSHARP):
        L.MgcgClearLastError()
        more = (dinv,) if jacobi else ()
        fn = L.SolveBicgstabJacobi if jacobi else L.SolveBicgstab
        st = fn(blas, sparse, None, vec, vec, vec, vec, vec, vec, vec, vec, v, s, t, rhat, *more, 28, 10, 1e-8, 0, 10, rule,
                C.byref(it), C.byref(res), C.byref(true), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for jacobi, who in ((False, "SolveBicgstab"), (True, "SolveBicgstabJacobi")):
        nulls = [dict(blas=None), dict(sparse=None), dict(v=None), dict(s=None), dict(t=None), dict(rhat=None)] + ([dict(dinv=None)] if jacobi else [])
        for kw in nulls:
            st, msg = call(jacobi, **kw)
            assert st == _lib.ERROR and f"{who}: null handle" in msg, (kw, msg)
        st, msg = call(jacobi, rule=_lib.RULE_HANDMADECL)
        assert st == _lib.ERROR and "max-norm" in msg and f"{who}:" in msg
        for rule in (-1, 5):
            st, msg = call(jacobi, rule=rule)
            assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
        for name in ("v", "s", "t", "rhat") + (("dinv",) if jacobi else ()):
            st, msg = call(jacobi, **{name: short})
            assert st == _lib.ERROR and f"the {name} vector holds 9 entries" in msg, (name, msg)
    # the several-ranks exports, called without a communicator, refuse the same way
    for jacobi in (False, True):
        L.MgcgClearLastError()
        more = (vec,) if jacobi else ()
        fn = L.SolveBicgstabJacobiParallel if jacobi else L.SolveBicgstabParallel
        st = fn(None, h, h, None, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, *more, 10, 10, 0, 28, 0, 9,
                1e-8, 0, 10, _lib.RULE_HANDMADECL, C.byref(it), C.byref(res), None, None, 0)
        assert st == _lib.ERROR and "max-norm" in _lib.last_error()
        L.MgcgClearLastError()
