"""MINRES on the host side (no GPU needed): the yardstick of tests/test_gpu_minres.py lives here and is checked against the true residual,
against classical CG and on the corner cases of the method; the library exports the two entry points and refuses bad arguments before it
asks for a device.

``minres_oracle`` is the loop of include/MgcgGpu.h (SolveMinres) in np.float64: every product goes into a named array or scalar before
the add that follows it, a matrix row is summed serially in stored order from +0.0 (``row_sums``), the scalars are evaluated in the
header's order, and every sum is a serial left-to-right sum (``serial_sum``), cut at ``parts`` and added in rank order.  Under
dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums
from tests.test_sreduce_host import classical_cg_iteration, randn_b, serial_sum, stop_decision, tridiagonal, with_b

DBL_BIG = 1.79e308


# --------------------------------------------------------------------------- the yardstick
def minres_oracle(s, shift=0.0, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, parts=None, x0=None, total=serial_sum):
    """(A - shift I) x = s.b from s.x (x0).  total(terms): the sum of one rank's terms (default: serial, left to right)."""
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    parts = [0, s.Count] if parts is None else [int(v) for v in parts]
    f = np.float64
    shift = f(shift)

    def sums(terms):
        acc = 0.0
        for lo, hi in zip(parts[:-1], parts[1:]):
            acc += total(terms[lo:hi]) if hi > lo else 0.0
        return f(acc)

    def true_residual(x):
        t = b - row_sums(e, c, ro, x)
        sx = shift * x
        return t + sx

    def closing(x, it, res, status, trace):
        r = true_residual(x)
        with np.errstate(all="ignore"):
            true = float(np.sqrt(sums(r * r)))
        return dict(x=x, r=r, iteration=it, residual=res, true_residual=true, status=status, trace=np.array(trace))

    with np.errstate(all="ignore"):
        x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
        r = true_residual(x)
        rr0 = sums(r * r)
        beta1 = np.sqrt(rr0)
        trace = [float(np.sqrt(rr0 / rr0)) if rule == _lib.RULE_VIENNACL else float(beta1)]
        if not (0.0 < rr0 <= DBL_BIG):
            return closing(x, 0, float(beta1), _lib.NONFINITE, trace)
        inv = f(1.0) / beta1
        v = r * inv
        vprev = w1 = w2 = None
        beta, cs, sn, dbar, eps, phibar = f(0.0), f(-1.0), f(0.0), f(0.0), f(0.0), beta1
        k = 0
        while True:
            q = row_sums(e, c, ro, v)
            delta = sums(v * q)
            # pass A
            dv = delta * v
            y = q - dv
            if k > 0:
                bv = beta * vprev
                y = y - bv
            yy = sums(y * y)
            # pass B
            alpha = delta - shift
            betan = np.sqrt(yy)
            oldeps = eps
            t1, t2 = cs * dbar, sn * alpha
            dl = t1 + t2
            t3, t4 = sn * dbar, cs * alpha
            gbar = t3 - t4
            eps_n = sn * betan
            cb = cs * betan
            dbar_n = -cb
            g2, b2 = gbar * gbar, betan * betan
            gamma = np.sqrt(g2 + b2)
            ig = f(1.0) / gamma
            cs_n, sn_n = gbar * ig, betan * ig
            phi, phibar_n = cs_n * phibar, sn_n * phibar
            if not (abs(gamma) <= DBL_BIG and abs(ig) <= DBL_BIG and abs(phi) <= DBL_BIG) or gamma == 0.0:     # breakdown, before this body's updates
                rr_old = phibar * phibar
                res = float(abs(phibar))
                trace.append(float(np.sqrt(rr_old / rr0)) if rule == _lib.RULE_VIENNACL else res)
                return closing(x, k + 1, res, _lib.NONFINITE, trace)
            eps, dbar, cs, sn, phibar = eps_n, dbar_n, cs_n, sn_n, phibar_n
            w = v
            if k >= 2:
                t = oldeps * w1
                w = w - t
            if k >= 1:
                t = dl * w2
                w = w - t
            w = w * ig
            pw = phi * w
            x = x + pw
            rr = phibar * phibar
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, rr, rr0)
            trace.append(shown)
            if betan == 0.0 and not stop:                  # the Krylov space is exhausted
                stop, status = True, _lib.OK
            if stop:
                return closing(x, k + 1, res, status, trace)
            ib = f(1.0) / betan
            vprev, v = v, y * ib
            w1, w2 = w2, w
            beta = betan
            k += 1


# --------------------------------------------------------------------------- what it is measured against
def _product(s, v):
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * v[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


def numpy_true_residual(s, shift, x):
    """|| b - (A - shift I) x ||_2 with numpy's own sums: independent of the yardstick's arithmetic."""
    return float(np.linalg.norm(s.b - _product(s, x) + shift * x))


def small(elements, cols, ro, x, b, name):
    return problems.LinearSystem(np.array(elements, dtype=np.float64), np.array(cols, dtype=np.int32), np.array(ro, dtype=np.int32),
                                 np.array(x, dtype=np.float64), np.array(b, dtype=np.float64), name)


def indefinite2():
    """[[1, 2], [2, 1]] (eigenvalues 3 and -1), which every CG loop refuses (tests/test_gpu_sreduce.py)."""
    return small([1.0, 2.0, 2.0, 1.0], [0, 1, 0, 1], [0, 2, 4], [0.25, -0.5], [1.0, -1.0], "indefinite2")


def singular2():
    """diag(1, 2), b = (1, 0): with shift 1 the shifted matrix is exactly singular on the Krylov space (gamma = 0 in body 0)."""
    return small([1.0, 2.0], [0, 1], [0, 1, 2], [0.0, 0.0], [1.0, 0.0], "singular2")


# (system, shift): the systems and shifts of tests/test_gpu_minres.py
SYSTEMS = {
    "poisson16": lambda: randn_b(problems.poisson(16, 16, 16), "poisson16"),
    "poisson12x10x7": lambda: randn_b(problems.poisson(12, 10, 7), "poisson12x10x7"),
    "random_spd5000": lambda: randn_b(problems.random_spd(5000), "random_spd5000"),
    "viennacl4000": lambda: randn_b(problems.viennacl_main(4000), "viennacl4000"),
    "poisson32x32": lambda: randn_b(problems.poisson(32, 32), "poisson32x32"),        # definite only: the comparison with CG
}
CASES = [("poisson16", 0.0), ("poisson16", 0.5), ("poisson12x10x7", 1.0), ("random_spd5000", 0.0), ("random_spd5000", 1.5),
         ("viennacl4000", 0.0), ("viennacl4000", 60.0)]
MAX_IT = 3000
_systems, _runs = {}, {}


def system(name):
    if name not in _systems:
        _systems[name] = SYSTEMS[name]()
    return _systems[name]


def run(name, shift, rel=1e-8):
    """The yardstick's run to a relative ``rel``, computed once and shared (nothing changes it)."""
    key = (name, shift, rel)
    if key not in _runs:
        s = system(name)
        _runs[key] = minres_oracle(s, shift, _lib.RULE_CSHARP, rel * float(np.linalg.norm(s.b)), max_it=MAX_IT)
    return _runs[key]


@pytest.mark.parametrize("name,shift", CASES)
def test_the_true_residual_is_within_the_stop_level(name, shift):
    s = system(name)
    level = 1e-8 * float(np.linalg.norm(s.b))
    o = run(name, shift)
    true = numpy_true_residual(s, shift, o["x"])
    print(f"{name} shift {shift:g}: {o['iteration']} iterations, recurrence {o['residual']:.3e}, true {true:.3e} = {true / level:.2f} x the stop level")
    assert o["status"] == _lib.OK and o["iteration"] >= 3
    assert o["residual"] < level
    assert true <= 1.0 * level
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    # the closing product's figure is the same quantity in the yardstick's own arithmetic: the two differ by the rounding of a row sum of
    # m + 2 terms in another order, at most (m + 2) eps (|A| |x| + |b| + |shift| |x|) per entry
    m = int(np.diff(s.RowOffsets).max())
    absA = problems.LinearSystem(np.abs(s.Elements), s.ColumnIndeces, s.RowOffsets, s.x, s.b, "abs")
    bound = (m + 2) * np.finfo(np.float64).eps * float(np.linalg.norm(_product(absA, np.abs(o["x"])) + np.abs(s.b) + abs(shift) * np.abs(o["x"])))
    assert abs(o["true_residual"] - true) <= bound
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("name,shift", CASES)
def test_the_trace_never_increases(name, shift):
    trace = run(name, shift)["trace"]
    assert len(trace) >= 4 and (np.diff(trace) <= 0.0).all()


@pytest.mark.parametrize("name", ["poisson16", "poisson32x32", "viennacl4000", "random_spd5000"])
def test_minres_needs_no_more_iterations_than_classical_cg(name):
    """MINRES minimises the norm the rule judges.  Its iteration k + 1 is the iterate of CG's body k: at most classical + 1."""
    s = system(name)
    goal = 1e-8 * float(np.linalg.norm(s.b))
    o = run(name, 0.0)
    classical = classical_cg_iteration(s, goal)
    print(f"{name}: MINRES {o['iteration']}, classical CG {classical}")
    assert o["status"] == _lib.OK and o["iteration"] <= classical + 1


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule):
    s = system("poisson16")
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else 1e-8 * float(np.linalg.norm(s.b))
    o = minres_oracle(start, 0.5, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 10
    zero = minres_oracle(s, 0.5, rule, tol, max_it=MAX_IT)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert (o["iteration"] == zero["iteration"] and np.array_equal(o["x"], zero["x"])) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2] and zero["trace"][0] == 1.0
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]


def test_the_iteration_cap_and_the_minimum_are_kept():
    s = system("poisson16")
    capped = minres_oracle(s, 0.5, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    tol = 1e-2 * float(np.linalg.norm(s.b))
    free = minres_oracle(s, 0.5, tol=tol, max_it=400)
    held = minres_oracle(s, 0.5, tol=tol, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5


def test_the_indefinite_2x2_matrix_is_solved():
    s = indefinite2()
    o = minres_oracle(s, 0.0, tol=1e-12)
    assert o["status"] == _lib.OK and o["iteration"] == 2
    assert np.allclose(o["x"], np.linalg.solve(np.array([[1.0, 2.0], [2.0, 1.0]]), s.b), rtol=1e-13, atol=0)
    assert numpy_true_residual(s, 0.0, o["x"]) < 1e-12


def test_a_singular_shifted_matrix_gives_nonfinite_and_the_callers_x_back():
    s = singular2()
    o = minres_oracle(s, 1.0, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], s.x)
    assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0
    # away from the eigenvalue the same system is solved in one body: b is an eigenvector
    ok = minres_oracle(s, 0.5, tol=1e-12)
    assert ok["status"] == _lib.OK and ok["iteration"] == 1 and np.array_equal(ok["x"], [2.0, 0.0])


def test_a_zero_right_hand_side_gives_nonfinite_at_iteration_0():
    s, _ = tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = minres_oracle(with_b(s, np.zeros(50), "b0"), 0.01, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


def test_an_exhausted_krylov_space_ends_the_loop_with_ok():
    s, _ = tridiagonal(1)
    o = minres_oracle(s, 0.0, tol=0.0, min_it=5, max_it=50)       # no rule would stop here: betan == 0 does
    assert o["status"] == _lib.OK and o["iteration"] == 1 and o["x"][0] == s.b[0] / 2.5 and o["residual"] == 0.0


def test_sums_are_cut_at_the_ranks_and_added_in_rank_order():
    s = system("random_spd5000")
    tol = 1e-8 * float(np.linalg.norm(s.b))
    one = run("random_spd5000", 1.5)
    cut = minres_oracle(s, 1.5, tol=tol, max_it=MAX_IT, parts=problems.partition_offsets(s.Count, 3))
    # another summation order, the same method: an indefinite Lanczos run is sensitive to it, so both solve the system and their counts
    # stay within 10 % (tests/test_gpu_minres.py has the measurement behind that figure)
    assert not np.array_equal(one["x"], cut["x"]) and cut["status"] == _lib.OK
    assert abs(one["iteration"] - cut["iteration"]) <= 0.1 * one["iteration"]
    assert numpy_true_residual(s, 1.5, cut["x"]) <= tol
    empty = minres_oracle(s, 1.5, tol=tol, max_it=MAX_IT, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- the library's host side
def test_the_two_symbols_are_exported_and_bound(hiplib):
    for name in ("SolveMinres", "SolveMinresParallel"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import minres, parallel

    assert "minres" in conjugategradient_amd.__all__ and "``minres``" in conjugategradient_amd.__doc__
    assert issubclass(minres.MinimalResidualGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    assert callable(parallel.ConjugateGradientRankGpu.SolveMinres)
    cg = minres.MinimalResidualGpu.__new__(minres.MinimalResidualGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    with pytest.raises(ValueError, match="max-norm"):
        minres.MinimalResidualGpu(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
    with pytest.raises(ValueError, match="finite"):
        minres.MinimalResidualGpu(10, 3, 0, 10, 1e-8, shift=float("inf"))


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

    def call(blas=h, sparse=h, r=vec, w1=vec, w2=vec, rule=_lib.RULE_CSHARP, shift=0.5):
        L.MgcgClearLastError()
        st = L.SolveMinres(blas, sparse, None, vec, vec, vec, vec, vec, vec, vec, r, w1, w2, 28, 10, shift, 1e-8, 0, 10, rule,
                           C.byref(it), C.byref(res), C.byref(true), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(w1=None), dict(w2=None)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "SolveMinres: null handle" in msg, (kw, msg)
    for shift in (float("nan"), float("inf"), -float("inf")):
        st, msg = call(shift=shift)
        assert st == _lib.ERROR and "SolveMinres: the shift is not finite" in msg, (shift, msg)
    st, msg = call(rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "SolveMinres" in msg
    for rule in (-1, 5):
        st, msg = call(rule=rule)
        assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
    st, msg = call(w1=short)
    assert st == _lib.ERROR and "the w1 vector holds 9 entries" in msg
    st, msg = call(w2=short)
    assert st == _lib.ERROR and "the w2 vector holds 9 entries" in msg
    st, msg = call(r=short)
    assert st == _lib.ERROR and "the r vector holds 9 entries" in msg
    # the several-ranks export, called without a communicator, refuses the same way
    L.MgcgClearLastError()
    st = L.SolveMinresParallel(None, h, h, None, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, 10, 10, 0, 28, 0, 9, float("nan"),
                               1e-8, 0, 10, _lib.RULE_CSHARP, C.byref(it), C.byref(res), None, None, 0)
    assert st == _lib.ERROR and "shift is not finite" in _lib.last_error()
    L.MgcgClearLastError()
