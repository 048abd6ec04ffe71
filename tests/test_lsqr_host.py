"""LSQR on the host side (no GPU needed): the yardstick of tests/test_gpu_lsqr.py lives here and is checked against numpy's dense least
squares, against scipy's lsqr and on the corner cases of the method; the library exports the entry point and refuses bad arguments before
it asks for a device.

``lsqr_oracle`` is the loop of include/MgcgGpu.h (MgcgSolveLsqr, "as computed") in np.float64: the two vectors of the bidiagonalisation stay
unnormalised, every product and quotient goes into a named array or scalar before the add that follows it, a matrix row is summed
serially in stored order from +0.0 (``row_sums``) -- A^T is ``transpose_arrays``' of tests/test_transpose_host.py, so row c of A^T is
summed in ascending stored position of A -- every square root is np.sqrt of two rounded squares and their sum, and every sum is a serial
left-to-right sum (``serial_sum``).  Under dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.product_cases import banded_rectangular, rectangular
from tests.test_mixed_host import row_sums
from tests.test_sreduce_host import serial_sum, stop_decision
from tests.test_transpose_host import transpose_arrays

DBL_BIG = 1.79e308
SEED = 20261018


# --------------------------------------------------------------------------- the yardstick
def lsqr_oracle(s, damp=0.0, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, total=serial_sum):
    """min || A x - s.b ||^2 + damp^2 || x ||^2 for a problems.LeastSquaresSystem, from x = 0.  total(terms): the sum of the terms
    (default: serial, left to right)."""
    f = np.float64
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz], dtype=np.int64)
    ro = np.asarray(s.RowOffsets, dtype=np.int64)
    b = np.asarray(s.b, dtype=np.float64)
    columns = int(s.Columns)
    et, ct, rot, _ = transpose_arrays(e, c, ro, columns)
    ct, rot = ct.astype(np.int64), rot.astype(np.int64)
    damp = f(damp)
    finite = lambda v: bool(abs(v) <= DBL_BIG)
    positive_finite = lambda v: bool(0.0 < v <= DBL_BIG)

    def A(v):
        return row_sums(e, c, ro, v)

    def At(u):
        return row_sums(et, ct, rot, u)

    def sums(terms):
        return f(total(terms))

    def closing(x, it, res, norm, status, trace):
        r = b - A(x)
        t = At(r)
        if damp != 0.0:
            l2 = damp * damp
            lx = l2 * x
            t = t - lx
        with np.errstate(all="ignore"):
            true, normal = float(np.sqrt(sums(r * r))), float(np.sqrt(sums(t * t)))
        return dict(x=x, r=r, t=t, iteration=it, residual=float(res), residual_norm=float(norm), true_residual=true, true_normal_residual=normal,
                    status=status, trace=np.array(trace, dtype=np.float64))

    with np.errstate(all="ignore"):
        x = np.zeros(columns)
        uh = b.copy()
        bb = sums(uh * uh)
        beta = np.sqrt(bb)
        t = At(uh)
        ib = f(1.0) / beta
        vh = t * ib
        vv = sums(vh * vh)
        alpha = np.sqrt(vv)
        g0 = alpha * beta
        gg0 = g0 * g0
        refused = True
        if not positive_finite(bb):
            g0, gg0 = beta, bb
        elif positive_finite(vv) and positive_finite(gg0):
            refused = False
        trace = [float(np.sqrt(gg0 / gg0)) if rule == _lib.RULE_VIENNACL else float(g0)]
        if refused:
            return closing(x, 0, g0, beta, _lib.NONFINITE, trace)
        phibar, rhobar, psi2, tr = beta, alpha, f(0.0), f(0.0)
        gg_last, norm = gg0, beta
        w = None
        k = 0
        while True:
            q = A(vh)
            # pass U
            ia = f(1.0) / alpha
            ab = alpha / beta
            qa = q * ia
            au = ab * uh
            uh_n = qa - au
            uu = sums(uh_n * uh_n)
            t = At(uh_n)
            # pass V
            betan = np.sqrt(uu)
            rhobar1, phibar1, psi2n = rhobar, phibar, psi2
            if damp != 0.0:
                r2, l2 = rhobar * rhobar, damp * damp
                rd = np.sqrt(r2 + l2)
                lr = damp / rd
                psi = lr * phibar
                cr = rhobar / rd
                phibar1 = cr * phibar
                pp = psi * psi
                psi2n = psi2 + pp
                rhobar1 = rd
            r2, b2 = rhobar1 * rhobar1, betan * betan
            rho = np.sqrt(r2 + b2)
            cs, sn = rhobar1 / rho, betan / rho
            phi, phibarn = cs * phibar1, sn * phibar1
            xs = phi / rho
            if not (finite(betan) and finite(rho) and finite(xs) and finite(phibarn) and finite(psi2n)) or rho == 0.0:    # breakdown, before this body's updates
                res = np.sqrt(gg_last)
                trace.append(float(np.sqrt(gg_last / gg0)) if rule == _lib.RULE_VIENNACL else float(res))
                return closing(x, k + 1, res, norm, _lib.NONFINITE, trace)
            uh = uh_n
            vn = vh * ia
            if k == 0:
                w = vn
            else:
                tw = tr * w
                w = vn - tw
            pw = xs * w
            x = x + pw
            if betan != 0.0:
                ibn = f(1.0) / betan
                tb = t * ibn
                bv = betan * vn
                vh = tb - bv
                vv = sums(vh * vh)
                alphan = np.sqrt(vv)
            else:
                alphan = f(0.0)
            # the scalar step
            theta = sn * alphan
            ca = cs * alphan
            rhobarn = -ca
            tr = theta / rho
            pa = abs(phibarn) * alphan
            g = pa * abs(cs)
            gg = g * g
            p2 = phibarn * phibarn
            norm = np.sqrt(p2 + psi2n)
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, gg, gg0)
            if g == 0.0:
                stop, status = True, _lib.OK
            trace.append(shown)
            if stop:
                return closing(x, k + 1, res, norm, status, trace)
            alpha, beta, phibar, rhobar, psi2, gg_last = alphan, betan, phibarn, rhobarn, psi2n, gg
            k += 1


# --------------------------------------------------------------------------- the cases (the issue's table; b = N(0,1) of `rows` entries)
def randn_rhs(system, columns, name):
    rows = len(system.RowOffsets) - 1
    return problems.least_squares(system, columns, np.random.default_rng(SEED).standard_normal(rows), name)


CASES = {
    "rect771x257": lambda: randn_rhs(rectangular(771, 257, 8, 1), 257, "rect771x257"),                 # tall, full rank
    "rect257x771": lambda: randn_rhs(rectangular(257, 771, 8, 2), 771, "rect257x771"),                 # wide, rank deficient: minimum-norm solution
    "rect1900x700x40": lambda: randn_rhs(rectangular(1900, 700, 40, 4), 700, "rect1900x700x40"),       # long rows: the lanes-per-row kernels on A
    "rect700x1900": lambda: randn_rhs(rectangular(700, 1900, 8, 1), 1900, "rect700x1900"),
    "banded1900x700": lambda: randn_rhs(banded_rectangular(1900, 700), 700, "banded1900x700"),         # empty rows
    "banded700x1900": lambda: randn_rhs(banded_rectangular(700, 1900), 1900, "banded700x1900"),        # empty rows and empty columns
    "rect300x7": lambda: randn_rhs(rectangular(300, 7, 3, 5), 7, "rect300x7"),                         # the Krylov space is exhausted
    "rect7x300": lambda: randn_rhs(rectangular(7, 300, 40, 6), 300, "rect7x300"),
    "convdiff12x10x8": lambda: randn_rhs(problems.convection_diffusion(12, 10, 8, c=(2.0, 1.0, 0.5), upwind=True), 960, "convdiff12x10x8"),   # square, A != A^T
    "nonsym1037": lambda: randn_rhs(problems.random_nonsymmetric(1037), 1037, "nonsym1037"),           # square
}
EXHAUSTED = ("rect300x7", "rect7x300")
NOT_EXHAUSTED = [n for n in CASES if n not in EXHAUSTED]
DAMPS = (0.0, 0.5)
REL = 1e-10
MAX_IT = 2000
_systems, _runs, _dense = {}, {}, {}


def system(name):
    if name not in _systems:
        _systems[name] = CASES[name]()
    return _systems[name]


def g0_of(s, damp=0.0):
    """g0 = alpha_1 beta_1 = || A^T b ||_2 up to rounding, with numpy's own sums (the level a relative rule refers to)."""
    return float(np.linalg.norm(s.to_scipy().T @ s.b))


def run(name, damp, rel=REL):
    """The yardstick's run to a relative ``rel`` in g, computed once and shared (nothing changes it)."""
    key = (name, damp, rel)
    if key not in _runs:
        s = system(name)
        _runs[key] = lsqr_oracle(s, damp, _lib.RULE_CSHARP, rel * g0_of(s), max_it=MAX_IT)
        for v in _runs[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _runs[key]


def dense_solution(name, damp):
    """(x, smallest eigenvalue of A^T A + damp^2 I on the space the solution lives in): numpy's lstsq on the dense matrix, augmented with
    damp * I; without damp lstsq returns the minimum-norm solution and the eigenvalue is the smallest nonzero sigma^2."""
    key = (name, damp)
    if key not in _dense:
        s = system(name)
        M = s.to_scipy().toarray()
        sv = np.linalg.svd(M, compute_uv=False)
        kept = sv[sv > 1e-10 * sv[0]]
        if damp:
            x = np.linalg.lstsq(np.vstack([M, damp * np.eye(s.Columns)]), np.concatenate([s.b, np.zeros(s.Columns)]), rcond=None)[0]
        else:
            x = np.linalg.lstsq(M, s.b, rcond=1e-10)[0]
        _dense[key] = (x, float(kept[-1] ** 2 + damp * damp), int(len(kept)), float(kept[0] / kept[-1]))
    return _dense[key]


def numpy_normal_residual(s, damp, x):
    """|| A^T (b - A x) - damp^2 x ||_2 with scipy's product and numpy's sums: independent of the yardstick's arithmetic."""
    M = s.to_scipy()
    return float(np.linalg.norm(M.T @ (s.b - M @ x) - damp * damp * x))


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_agrees_with_dense_least_squares_and_with_scipy(name, damp):
    """The stop leaves g <= 1e-10 g0.  The error of x then obeys (A^T A + damp^2 I)(x* - x) = A^T (b - A x) - damp^2 x with both sides in the
    range of A^T (x is a combination of the v_k), so || x - x* || <= || normal residual || / lambda_min, lambda_min the smallest eigenvalue
    of A^T A + damp^2 I on that range.  Asserted with the true normal residual allowed 2 x the stop level (the recurrence's g is an
    estimate; the test below has the two equal to three digits), plus the same again for lstsq's own error."""
    import scipy.sparse.linalg as spla

    s = system(name)
    o = run(name, damp)
    x_dense, lam_min, rank, cond = dense_solution(name, damp)
    level = REL * g0_of(s)
    err = float(np.linalg.norm(o["x"] - x_dense))
    rel_err = err / float(np.linalg.norm(x_dense))
    print(f"{name} damp {damp:g}: {o['iteration']} bodies, rank {rank}, cond {cond:.3g}, g {o['residual']:.3e} = {o['residual'] / level:.3f} x level, "
          f"true normal residual {o['true_normal_residual']:.3e}, residual norm estimate {o['residual_norm']:.6e} true {o['true_residual']:.6e}, "
          f"|x - x_lstsq| / |x| {rel_err:.2e}")
    assert o["status"] == _lib.OK and len(o["trace"]) == o["iteration"] + 1
    assert o["residual"] < level or o["residual"] == 0.0 or name in EXHAUSTED
    assert err <= 4.0 * level / lam_min
    assert rel_err <= 1e-8
    # scipy's lsqr to its tightest tolerances: the same minimiser
    xs = spla.lsqr(s.to_scipy(), s.b, damp=damp, atol=1e-14, btol=1e-14, conlim=0.0, iter_lim=20 * MAX_IT)[0]
    assert float(np.linalg.norm(o["x"] - xs)) <= 4.0 * level / lam_min + 1e-9 * float(np.linalg.norm(xs))
    # the closing figures are the yardstick's own arithmetic of independent quantities
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"])) and o["true_normal_residual"] == math.sqrt(serial_sum(o["t"] * o["t"]))
    M = s.to_scipy()
    assert abs(o["true_residual"] - float(np.linalg.norm(s.b - M @ o["x"]))) <= 1e-12 * float(np.linalg.norm(s.b))
    # the residual norm's estimate: || b - A x ||, with damp sqrt(|| b - A x ||^2 + damp^2 || x ||^2).  phibar starts as || b || and is
    # multiplied down, so its rounding is relative to || b ||, not to itself (a consistent square system: 6e-9 of || b || = 31)
    damped = math.sqrt(float(np.linalg.norm(s.b - M @ o["x"])) ** 2 + (damp * float(np.linalg.norm(o["x"]))) ** 2)
    assert abs(o["residual_norm"] - damped) <= 1e-8 * damped + 1e-12 * float(np.linalg.norm(s.b))


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", NOT_EXHAUSTED)
def test_g_is_the_true_normal_residual_to_three_digits(name, damp):
    s = system(name)
    o = run(name, damp)
    true = numpy_normal_residual(s, damp, o["x"])
    print(f"{name} damp {damp:g}: g {o['residual']:.6e}, true {true:.6e}, ratio {true / o['residual']:.5f}")
    assert abs(true / o["residual"] - 1.0) <= 5e-3
    assert abs(o["true_normal_residual"] - true) <= 1e-3 * true
    assert true <= 2.0 * REL * g0_of(s)


@pytest.mark.parametrize("name", ["rect771x257", "convdiff12x10x8"])
def test_the_g_trace_falls_to_the_stop_level(name):
    o = run(name, 0.0)
    trace = o["trace"]
    assert len(trace) >= 10 and trace[0] == trace.max() and trace[-1] == o["residual"] == trace.min()
    # LSQR does not minimise g, so the trace is not monotone; it must still fall by ten orders and every entry must be a finite positive number
    assert np.isfinite(trace).all() and (trace > 0.0).all() and trace[-1] < 1e-10 * trace[0] <= trace[-2]


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule):
    s = system("rect771x257")
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else 1e-8 * g0_of(s)
    o = lsqr_oracle(s, 0.5, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 10
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][0] == 1.0 and o["trace"][-1] < tol <= o["trace"][-2]
    else:
        assert o["residual"] < tol <= o["trace"][-2] and o["trace"][-1] == o["residual"]
    # the relative rule and the absolute ones stop at the same body when their levels are the same
    assert o["iteration"] == lsqr_oracle(s, 0.5, _lib.RULE_CSHARP, 1e-8 * g0_of(s), max_it=MAX_IT)["iteration"]
    # x starts from 0 under every rule: nothing of the system but A and b is read
    assert numpy_normal_residual(s, 0.5, o["x"]) <= 2e-8 * g0_of(s)


def test_the_iteration_cap_and_the_minimum_are_kept():
    s = system("rect771x257")
    capped = lsqr_oracle(s, 0.0, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    tol = 1e-3 * g0_of(s)
    free = lsqr_oracle(s, 0.0, tol=tol)
    held = lsqr_oracle(s, 0.0, tol=tol, min_it=free["iteration"] + 5)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    assert np.array_equal(held["trace"][: free["iteration"] + 1], free["trace"])


def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0():
    s = system("rect771x257")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = lsqr_oracle(problems.least_squares(s, s.Columns, np.zeros(s.Rows)), 0.0, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert zero["residual_norm"] == 0.0 and zero["true_residual"] == 0.0 and zero["true_normal_residual"] == 0.0
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


def orthogonal_rhs(s):
    """A nonzero b with A^T b == 0 exactly: nonzero only in rows that store nothing."""
    empty = np.diff(s.RowOffsets) == 0
    assert empty.sum() >= 2
    return np.where(empty, 1.0 + np.arange(s.Rows) % 3, 0.0)


def test_a_right_hand_side_orthogonal_to_the_range_gives_nonfinite_at_iteration_0():
    s = system("banded1900x700")
    b = orthogonal_rhs(s)
    o = lsqr_oracle(problems.least_squares(s, s.Columns, b), 0.0, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 0 and o["residual"] == 0.0 and not o["x"].any()
    # x = 0 IS the least-squares solution: the residual is b itself and the normal residual is zero
    assert o["residual_norm"] == o["true_residual"] == math.sqrt(serial_sum(b * b)) and o["true_normal_residual"] == 0.0 and list(o["trace"]) == [0.0]


def test_a_1_by_1_system_is_solved_in_one_body():
    s = problems.LeastSquaresSystem(np.array([4.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([2.0]), 1, "1x1")
    o = lsqr_oracle(s, 0.0, tol=0.0, min_it=5, max_it=50)                # no rule would stop here: g == 0 does
    assert o["status"] == _lib.OK and o["iteration"] == 1 and o["x"][0] == 0.5 and o["residual"] == 0.0 and o["true_residual"] == 0.0
    d = lsqr_oracle(s, 3.0, tol=0.0, min_it=5, max_it=50)                # damped: x = a b / (a^2 + damp^2)
    assert d["status"] == _lib.OK and d["iteration"] == 1 and abs(d["x"][0] - 8.0 / 25.0) <= 1e-16
    assert abs(d["residual_norm"] - math.sqrt((2.0 - 4.0 * 8.0 / 25.0) ** 2 + 9.0 * (8.0 / 25.0) ** 2)) <= 1e-15


@pytest.mark.parametrize("name", EXHAUSTED)
def test_an_exhausted_krylov_space_ends_the_loop(name):
    """At most min(rows, columns) bodies span the space: the loop ends by g == 0 exactly or by the rule on a g at rounding level."""
    s = system(name)
    o = run(name, 0.0)
    assert o["status"] == _lib.OK and o["iteration"] <= min(s.Rows, s.Columns) + 1
    assert numpy_normal_residual(s, 0.0, o["x"]) <= 1e-10 * g0_of(s)


# --------------------------------------------------------------------------- the library's host side
def test_the_symbol_is_exported_and_bound(hiplib):
    assert hasattr(hiplib, "MgcgSolveLsqr") and "MgcgSolveLsqr" in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3                                    # the addition is additive


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import lsqr

    assert "lsqr" in conjugategradient_amd.__all__ and "``lsqr``" in conjugategradient_amd.__doc__
    assert issubclass(lsqr.LeastSquaresGpu, conjugategradient_amd.solver.ConjugateGradientGpu)
    for name in ("Initialize", "Solve", "Read", "ReadResidual", "ReadNormalResidual", "load"):
        assert callable(getattr(lsqr.LeastSquaresGpu, name))
    cg = lsqr.LeastSquaresGpu.__new__(lsqr.LeastSquaresGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    with pytest.raises(ValueError, match="max-norm"):
        lsqr.LeastSquaresGpu(10, 4, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
    for damp in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="damp"):
            lsqr.LeastSquaresGpu(10, 4, 3, 0, 10, 1e-8, damp=damp)
    s = problems.sparse_rectangular(50, 20, 4, seed=3)
    assert (s.Rows, s.Columns, s.nnz) == (50, 20, 200) and s.b.shape == (50,) and int(s.ColumnIndeces.max()) < 20
    assert (np.diff(s.ColumnIndeces.reshape(50, 4), axis=1) >= 0).all() and s.to_scipy().shape == (50, 20)


def test_the_class_hands_its_own_native_call_what_the_header_declares(monkeypatch):
    """LeastSquaresGpu does not go through ConjugateGradientGpu._native_solve (two matrices, two sizes): its call is pinned here with the
    recording fake of tests/test_python_calls_host.py, argument by argument, and so is what it makes of the answer."""
    from conjugategradient_amd import lsqr
    from conjugategradient_amd.solver import ApplicationException
    from tests.test_python_calls_host import _BYREF, FakeLibrary, STATUSES

    class Fake(FakeLibrary):
        """FakeLibrary answers two double cells; MgcgSolveLsqr has four: 0.25, 0.5, 0.75, 1.0 here, 5 into the int cell, the trace 1, 1/2, ..."""

        def _answer(self, name, args):
            return self._solve(name, args) if name == "MgcgSolveLsqr" else super()._answer(name, args)

        def _solve(self, name, args):
            self.solves.append((name, [f"{type(a._obj).__name__}({a._obj.value})" if isinstance(a, _BYREF) else "<pointer>" if isinstance(a, C.c_void_p) else a for a in args]))
            doubles = iter((0.25, 0.5, 0.75, 1.0))
            for cell in (a._obj for a in args if isinstance(a, _BYREF)):
                cell.value = 5 if isinstance(cell, C.c_int) else next(doubles)
            out = C.cast(args[-2], C.POINTER(C.c_double))
            for i in range(args[-1]):
                out[i] = 0.5 ** i
            self.error = self.message.encode()
            return self.status

    s = problems.sparse_rectangular(9, 4, 3, seed=1)
    for status, raised in (("ok", None), ("maxit", ApplicationException), ("nonfinite", _lib.MgcgError), ("error_said", _lib.MgcgError)):
        fake = Fake("ok")
        monkeypatch.setattr(_lib, "_LIB", fake)
        cg = lsqr.LeastSquaresGpu(9, 4, 3, 0, 10, 1e-8, rule=_lib.RULE_CSHARP, damp=0.25).load(s)
        try:
            fake.recording = True
            cg.Initialize()
            transposes = [c for c in fake.calls if c.startswith("MgcgCsrTranspose(")]
            assert transposes == ["MgcgCsrTranspose(<CreateBlas>, <CreateSparse>, <double[27]>, <int[10]>, <int[27]>, 27, 9, 4, <double[27]>, <int[5]>, <int[27]>, None)"]
            fake.status, fake.message = STATUSES[status]
            try:
                cg.Solve(trace=True, traceCapacity=3)
                assert raised is None
            except Exception as e:
                assert raised is not None and type(e) is raised, e
            fake.recording = False
            (export, args), = fake.solves
            assert export == "MgcgSolveLsqr" and len(args) == len(_lib.SIGNATURES["MgcgSolveLsqr"][1]) == 31
            v = lambda name: getattr(cg, name).Ptr
            assert args[:3] == [cg.cublas, cg.cusparse, cg.matDescr]
            assert args[3:16] == [v("vectorA"), v("vectorRowOffsets"), v("vectorColumnIndeces"), v("vectorAT"), v("vectorRowOffsetsT"), v("vectorColumnIndecesT"),
                                  v("vectorX"), v("vectorB"), v("vectorU"), v("vectorV"), v("vectorW"), v("vectorQ"), v("vectorT")]
            assert [(getattr(cg, n).size) for n in ("vectorX", "vectorB", "vectorU", "vectorV", "vectorW", "vectorQ", "vectorT", "vectorRowOffsets", "vectorRowOffsetsT")] == [4, 9, 9, 4, 4, 9, 4, 10, 5]
            assert args[16:24] == [27, 9, 4, 0.25, 1e-8, 0, 10, _lib.RULE_CSHARP]
            assert args[24:29] == ["c_int(0)", "c_double(nan)", "c_double(nan)", "c_double(nan)", "c_double(nan)"] and args[29:] == ["<pointer>", 3]
            assert (cg.Iteration, cg.Residual, cg.ResidualNorm, cg.TrueResidual, cg.TrueNormalResidual, cg.status) == (5, 0.25, 0.5, 0.75, 1.0, STATUSES[status][0])
            assert list(cg.trace) == [1.0, 0.5, 0.25]
        finally:                                         # the object's vectors go while the fake is still the library
            cg.Dispose()
    monkeypatch.undo()


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    it, res = C.c_int(0), C.c_double(0.0)
    handle = C.create_string_buffer(4096)                  # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    rows, columns, nnz = 10, 6, 28
    heads = {n: _VectorHead(None, n, -1, b"") for n in (28, 27, 11, 10, 9, 7, 6, 5)}
    v = {n: C.addressof(head) for n, head in heads.items()}
    names = ("e", "ro", "ci", "et", "rot", "cit", "x", "b", "u", "v", "w", "q", "t")
    good = dict(e=v[28], ro=v[11], ci=v[28], et=v[28], rot=v[7], cit=v[28], x=v[6], b=v[10], u=v[10], v=v[6], w=v[6], q=v[10], t=v[6])

    def call(blas=h, sparse=h, rule=_lib.RULE_CSHARP, damp=0.5, rows=rows, columns=columns, nnz=nnz, **vectors):
        L.MgcgClearLastError()
        a = dict(good, **vectors)
        st = L.MgcgSolveLsqr(blas, sparse, None, *(a[n] for n in names), nnz, rows, columns, damp, 1e-8, 0, 10, rule,
                         C.byref(it), C.byref(res), None, None, None, None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "MgcgSolveLsqr: null handle" in msg, (kw, msg)
    for n in names:
        st, msg = call(**{n: None})
        assert st == _lib.ERROR and "MgcgSolveLsqr: null vector handle" in msg, (n, msg)
    for kw in (dict(rows=0), dict(columns=0), dict(rows=-3), dict(nnz=-1)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "MgcgSolveLsqr: bad sizes" in msg, (kw, msg)
    for damp in (-0.5, float("nan"), float("inf"), -float("inf")):
        st, msg = call(damp=damp)
        assert st == _lib.ERROR and "MgcgSolveLsqr: damp is negative or not finite" in msg, (damp, msg)
    st, msg = call(rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "MgcgSolveLsqr" in msg
    for rule in (-1, 5):
        st, msg = call(rule=rule)
        assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
    # a vector too small for its role: "rows" or "columns" says which dimension it must hold
    for n, of, short, need in (("x", "columns", 5, 6), ("v", "columns", 5, 6), ("w", "columns", 5, 6), ("t", "columns", 5, 6),
                               ("b", "rows", 9, 10), ("u", "rows", 9, 10), ("q", "rows", 9, 10)):
        st, msg = call(**{n: v[short]})
        assert st == _lib.ERROR and f"MgcgSolveLsqr: the {n} vector holds {short} entries, the matrix has {need} {of}" in msg, (n, msg)
    for n, which in (("e", "A"), ("ci", "A"), ("et", "A^T"), ("cit", "A^T")):
        st, msg = call(**{n: v[27]})
        assert st == _lib.ERROR and f"a vector of {which} is smaller than the matrix" in msg, (n, msg)
    st, msg = call(ro=v[10])
    assert st == _lib.ERROR and "a vector of A is smaller than the matrix" in msg
    st, msg = call(rot=v[6])
    assert st == _lib.ERROR and "a vector of A^T is smaller than the matrix" in msg
