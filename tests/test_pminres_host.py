"""Preconditioned MINRES on the host side (no GPU needed): the yardstick of tests/test_gpu_pminres.py lives here and is checked against the
true residual in the norm the method minimises, against plain MINRES and on the corner cases of the method; the library exports the three
entry points and refuses bad arguments before it asks for a device.

``pminres_oracle`` is the loop of include/MgcgGpu.h (SolveMinresJacobi / SolveMinresMg) in np.float64, built as ``minres_oracle``
(tests/test_minres_host.py) is: every product goes into a named array or scalar before the add that follows it, a matrix row is summed
serially in stored order from +0.0 (``row_sums``), the scalars are evaluated in the header's order, and every sum is a serial left-to-right
sum (``serial_sum``), cut at ``parts`` and added in rank order.  ``minv`` applies M^-1: ``lambda r: dinv * r`` or ``Hierarchy(...).apply``
(tests/test_amg_host.py).  Under dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import Hierarchy, csr_of, diagonal_inverse, graph_laplacian
from tests.test_minres_host import DBL_BIG, _product, minres_oracle, singular2, system
from tests.test_mixed_host import row_sums
from tests.test_sreduce_host import serial_sum, stop_decision, tridiagonal, with_b


# --------------------------------------------------------------------------- the yardstick
def pminres_oracle(s, shift=0.0, minv=None, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, parts=None, x0=None, total=serial_sum):
    """(A - shift I) x = s.b from s.x (x0) with the preconditioner z = minv(r).  total(terms): the sum of one rank's terms (default: serial,
    left to right).  ``residual`` and ``trace`` are the recurrence's figure, the residual in the M^-1 norm; ``true_residual`` the 2-norm."""
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
        r2 = true_residual(x)
        z = minv(r2)
        bz = sums(r2 * z)
        beta1 = np.sqrt(bz)
        trace = [float(np.sqrt(bz / bz)) if rule == _lib.RULE_VIENNACL else float(beta1)]
        if not (0.0 < bz <= DBL_BIG):
            return closing(x, 0, float(beta1), _lib.NONFINITE, trace)
        inv = f(1.0) / beta1
        v = z * inv
        vv = sums(v * v)
        r1 = w1 = w2 = None
        beta, oldb, cs, sn, dbar, eps, phibar = beta1, f(0.0), f(-1.0), f(0.0), f(0.0), f(0.0), beta1
        k = 0

        def refused():                                     # before this body's updates: the last judged residual once more
            rr_old = phibar * phibar
            res = float(abs(phibar))
            trace.append(float(np.sqrt(rr_old / bz)) if rule == _lib.RULE_VIENNACL else res)
            return closing(x, k + 1, res, _lib.NONFINITE, trace)

        while True:
            q = row_sums(e, c, ro, v)
            vq = sums(v * q)
            # pass A
            sv = shift * vv
            alpha = vq - sv
            y = q
            if shift != 0.0:
                t = shift * v
                y = q - t
            if k > 0:
                c1 = beta / oldb
                t = c1 * r1
                y = y - t
            c2 = alpha / beta
            t2 = c2 * r2
            rn = y - t2
            z = minv(rn)
            rz = sums(rn * z)
            # pass B
            if not (0.0 <= rz <= DBL_BIG):
                return refused()
            betan = np.sqrt(rz)
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
            if not (abs(gamma) <= DBL_BIG and abs(ig) <= DBL_BIG and abs(phi) <= DBL_BIG) or gamma == 0.0:     # breakdown
                return refused()
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
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, rr, bz)
            trace.append(shown)
            if betan == 0.0 and not stop:                  # the Krylov space is exhausted
                stop, status = True, _lib.OK
            if stop:
                return closing(x, k + 1, res, status, trace)
            ib = f(1.0) / betan
            v = z * ib
            vv = sums(v * v)
            r1, r2 = r2, rn
            w1, w2 = w2, w
            oldb, beta = beta, betan
            k += 1


# --------------------------------------------------------------------------- systems, preconditioners, shared runs
def graph12():
    s = graph_laplacian(12, 5)
    return with_b(s, np.random.default_rng(1).standard_normal(s.Count), "graph-laplacian-12-randn")


_cache = {}


def psystem(name):
    if name == "graph12":
        if name not in _cache:
            _cache[name] = graph12()
        return _cache[name]
    return system(name)


def jacobi_of(s):
    dinv = diagonal_inverse(*csr_of(s))
    return lambda r: dinv * r


def preconditioner(name, kind):
    """The callable z = M^-1 r, built once per (system, kind): 'jacobi' or 'vcycle' (the yardstick hierarchy with its defaults)."""
    key = ("M", name, kind)
    if key not in _cache:
        s = psystem(name)
        _cache[key] = jacobi_of(s) if kind == "jacobi" else Hierarchy(*csr_of(s)).apply
    return _cache[key]


def m_norm(minv, r):
    """sqrt(r . M^-1 r) with numpy's own sums."""
    return float(np.sqrt(r @ minv(r)))


def numpy_residual_vector(s, shift, x):
    return s.b - _product(s, x) + shift * x


# (system, shift, preconditioner): the cases of tests/test_gpu_pminres.py
CASES = [("viennacl4000", 0.0, "jacobi"), ("viennacl4000", 60.0, "jacobi"), ("random_spd5000", 0.0, "jacobi"), ("random_spd5000", 1.5, "jacobi"),
         ("graph12", 0.0, "jacobi"), ("graph12", 20.0, "jacobi"), ("graph12", 0.0, "vcycle"), ("graph12", 20.0, "vcycle")]
MAX_IT = 3000


def stop_level(name, kind, rel=1e-8):
    """rel x the M^-1 norm of b: every system here starts from x = 0, so this is rel x beta1 up to the order of a sum."""
    s = psystem(name)
    assert not s.x.any()
    return rel * m_norm(preconditioner(name, kind), np.asarray(s.b))


def run(name, shift, kind, rel=1e-8):
    """The yardstick's run to a relative ``rel`` in the M^-1 norm, computed once and shared (nothing changes it)."""
    key = ("run", name, shift, kind, rel)
    if key not in _cache:
        _cache[key] = pminres_oracle(psystem(name), shift, preconditioner(name, kind), _lib.RULE_CSHARP, stop_level(name, kind, rel), max_it=MAX_IT)
    return _cache[key]


def plain(name, shift, rel=1e-8):
    key = ("plain", name, shift, rel)
    if key not in _cache:
        s = psystem(name)
        _cache[key] = minres_oracle(s, shift, _lib.RULE_CSHARP, rel * float(np.linalg.norm(s.b)), max_it=MAX_IT)
    return _cache[key]


# --------------------------------------------------------------------------- 1. the M^-1 norm at the stop ; 2. the trace
@pytest.mark.parametrize("name,shift,kind", CASES)
def test_the_true_residual_in_the_m_norm_is_within_the_stop_level(name, shift, kind):
    """The recurrence's phibar against sqrt(r . M^-1 r) of the numpy residual of x.  Measured for this yardstick, true / stop level, in the
    order of CASES: 0.08, 0.47, 0.85, 0.69, 0.95, 0.94, 0.67, 0.63 -- the recurrence and the numpy figure agree to three digits or more,
    and the last body lands that far below the level -- so the margin is 1.0, as for plain MINRES (tests/test_minres_host.py).  The 2-norm
    is another matter: relative to || b ||_2 it is 0.54 to 2.22 x the relative M^-1 norm at the stop (printed)."""
    s = psystem(name)
    minv = preconditioner(name, kind)
    level = stop_level(name, kind)
    o = run(name, shift, kind)
    r = numpy_residual_vector(s, shift, o["x"])
    true_m = m_norm(minv, r)
    true_2 = float(np.linalg.norm(r))
    rel_m, rel_2 = true_m / m_norm(minv, np.asarray(s.b)), true_2 / float(np.linalg.norm(s.b))
    print(f"{name} shift {shift:g} {kind}: {o['iteration']} iterations, recurrence {o['residual']:.3e}, true (M^-1 norm) {true_m:.3e} = "
          f"{true_m / level:.4f} x the stop level; relative 2-norm / relative M^-1 norm = {rel_2 / rel_m:.2f}")
    assert o["status"] == _lib.OK and o["iteration"] >= 3
    assert o["residual"] < level
    assert true_m <= 1.0 * level
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    # the closing product's figure is the plain 2-norm, the same quantity in the yardstick's own arithmetic (the bound of tests/test_minres_host.py)
    m = int(np.diff(s.RowOffsets).max())
    absA = problems.LinearSystem(np.abs(s.Elements), s.ColumnIndeces, s.RowOffsets, s.x, s.b, "abs")
    bound = (m + 2) * np.finfo(np.float64).eps * float(np.linalg.norm(_product(absA, np.abs(o["x"])) + np.abs(s.b) + abs(shift) * np.abs(o["x"])))
    assert abs(o["true_residual"] - true_2) <= bound
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("name,shift,kind", CASES)
def test_the_trace_never_increases(name, shift, kind):
    trace = run(name, shift, kind)["trace"]
    assert len(trace) >= 4 and (np.diff(trace) <= 0.0).all()


# --------------------------------------------------------------------------- 3. the identity preconditioner
@pytest.mark.parametrize("name,shift", [("viennacl4000", 0.0), ("viennacl4000", 60.0), ("random_spd5000", 0.0), ("random_spd5000", 1.5)])
def test_the_identity_preconditioner_is_plain_minres(name, shift):
    """dinv = 1: the same Krylov space and the same norm, another arrangement of the recurrence (alpha from v.q and v.v, r1 and r2 not
    normalised): the count within one iteration, x to 1e-10 relative.  Tolerance 1e-12 of || b ||, so that the iteration the two may
    differ by moves x by far less than the bound.  The graph Laplacian is not among the systems: the count of plain MINRES itself moves
    from 569 to 476 there when its serial sums are replaced by numpy's pairwise ones, so a count within one says nothing on it."""
    s = psystem(name)
    tol = 1e-12 * float(np.linalg.norm(s.b))
    ref = minres_oracle(s, shift, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    one = pminres_oracle(s, shift, lambda r: 1.0 * r, _lib.RULE_CSHARP, tol, max_it=MAX_IT)
    distance = float(np.linalg.norm(one["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    print(name, shift, "iterations", one["iteration"], ref["iteration"], "distance", distance)
    assert one["status"] == ref["status"] == _lib.OK
    assert abs(one["iteration"] - ref["iteration"]) <= 1
    assert distance <= 1e-10


# --------------------------------------------------------------------------- 4. the iteration cuts
@pytest.mark.parametrize("name,shift,kind,fraction", [("viennacl4000", 60.0, "jacobi", 0.25), ("viennacl4000", 0.0, "jacobi", 0.25),
                                                       ("graph12", 20.0, "vcycle", 0.5)])
def test_the_preconditioner_cuts_the_iterations(name, shift, kind, fraction):
    """Each run to a relative 1e-8 in the norm its recurrence sees."""
    o, p = run(name, shift, kind), plain(name, shift)
    print(f"{name} shift {shift:g}: {kind} {o['iteration']}, plain {p['iteration']}")
    assert o["status"] == p["status"] == _lib.OK
    assert o["iteration"] <= fraction * p["iteration"]


# --------------------------------------------------------------------------- 5. corner cases
def test_a_negative_definite_preconditioner_gives_nonfinite_at_iteration_0():
    s = psystem("random_spd5000")
    start = with_b(s, s.b, "x0")
    start.x[:] = 0.25
    o = pminres_oracle(start, 1.5, lambda r: -1.0 * r, tol=1e-8)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 0 and np.array_equal(o["x"], start.x)
    assert len(o["trace"]) == 1 and math.isnan(o["trace"][0]) and math.isnan(o["residual"])
    assert o["true_residual"] > 0.0


def test_a_preconditioner_that_turns_indefinite_inside_the_loop_gives_nonfinite():
    """M = diag(1, -1e-3) on diag(1, 2), b = (1, 1): bz = 0.999 > 0, and body 0's rn.z is negative."""
    s = problems.LinearSystem(np.array([1.0, 2.0]), np.array([0, 1], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.zeros(2), np.array([1.0, 1.0]), "d2")
    d = np.array([1.0, -1e-3])
    o = pminres_oracle(s, 0.0, lambda r: d * r, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and not o["x"].any()
    assert len(o["trace"]) == 2 and o["trace"][0] == o["trace"][1] == o["residual"]


def test_a_singular_shifted_matrix_and_a_zero_right_hand_side_give_nonfinite():
    s = singular2()
    one = lambda r: 1.0 * r                                                # noqa: E731
    o = pminres_oracle(s, 1.0, one, tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], s.x)
    assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0
    # ... with its own diagonal as well
    o = pminres_oracle(s, 1.0, jacobi_of(s), tol=1e-12)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], s.x)
    t, _ = tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = pminres_oracle(with_b(t, np.zeros(50), "b0"), 0.01, jacobi_of(t), rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)


def test_an_exhausted_krylov_space_ends_the_loop_with_ok():
    s, _ = tridiagonal(1)
    o = pminres_oracle(s, 0.0, jacobi_of(s), tol=0.0, min_it=5, max_it=50)       # no rule would stop here: betan == 0 does
    # in exact arithmetic body 0's rn is 0; rounded, 2.5 v - (alpha / beta) r2 may leave one unit in the last place, and body 1 ends the loop
    assert o["status"] == _lib.OK and o["iteration"] in (1, 2) and o["residual"] == 0.0 and len(o["trace"]) == o["iteration"] + 1
    assert abs(o["x"][0] - s.b[0] / 2.5) <= 2 * np.finfo(np.float64).eps * abs(s.b[0] / 2.5)


def test_the_cap_the_minimum_and_the_four_rules():
    s = psystem("graph12")
    minv = preconditioner("graph12", "jacobi")
    level = stop_level("graph12", "jacobi")
    capped = pminres_oracle(s, 20.0, minv, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    free = pminres_oracle(s, 0.0, minv, tol=1e6 * level, max_it=400)
    held = pminres_oracle(s, 0.0, minv, tol=1e6 * level, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    for rule in (_lib.RULE_NATIVE, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL):
        tol = 1e-2 if rule == _lib.RULE_VIENNACL else 1e6 * level
        o = pminres_oracle(s, 0.0, minv, rule, tol, max_it=400)
        assert o["status"] == _lib.OK and o["iteration"] >= 3
        assert (o["trace"][-1] < tol <= o["trace"][-2] and o["trace"][0] == 1.0) if rule == _lib.RULE_VIENNACL else o["residual"] < tol


def test_sums_are_cut_at_the_ranks_and_added_in_rank_order():
    s = psystem("random_spd5000")
    minv = preconditioner("random_spd5000", "jacobi")
    level = stop_level("random_spd5000", "jacobi")
    one = run("random_spd5000", 1.5, "jacobi")
    cut = pminres_oracle(s, 1.5, minv, tol=level, max_it=MAX_IT, parts=problems.partition_offsets(s.Count, 3))
    # another summation order, the same method: both solve the system, and their counts stay within 10 % (tests/test_minres_host.py)
    assert not np.array_equal(one["x"], cut["x"]) and cut["status"] == _lib.OK
    assert abs(one["iteration"] - cut["iteration"]) <= 0.1 * one["iteration"]
    assert m_norm(minv, numpy_residual_vector(s, 1.5, cut["x"])) <= level
    empty = pminres_oracle(s, 1.5, minv, tol=level, max_it=MAX_IT, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- 6. the library's host side
def test_the_three_symbols_are_exported_and_bound(hiplib):
    for name in ("SolveMinresJacobi", "SolveMinresJacobiParallel", "SolveMinresMg"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3


def test_python_surface_imports_without_a_gpu():
    from conjugategradient_amd import amg, minres, multigrid, parallel

    assert issubclass(minres.MinimalResidualJacobiGpu, minres.MinimalResidualGpu)
    assert callable(multigrid.ConjugateGradientMgGpu.SolveMinres)
    assert amg.ConjugateGradientAmgGpu.SolveMinres is multigrid.ConjugateGradientMgGpu.SolveMinres
    assert callable(parallel.ConjugateGradientRankGpu.SolveMinresJacobi)
    for cls in (minres.MinimalResidualJacobiGpu, multigrid.ConjugateGradientMgGpu.SolveMinres):
        assert "M^-1 norm" in cls.__doc__ and "TrueResidual" in cls.__doc__
    cg = minres.MinimalResidualJacobiGpu.__new__(minres.MinimalResidualJacobiGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    with pytest.raises(ValueError, match="max-norm"):
        minres.MinimalResidualJacobiGpu(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
    with pytest.raises(ValueError, match="finite"):
        minres.MinimalResidualJacobiGpu(10, 3, 0, 10, 1e-8, shift=float("nan"))


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    """The refusals that need a hierarchy (its row count, its ranks) are in tests/test_gpu_pminres.py: there is no hierarchy without a device."""
    L = hiplib
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    handle = C.create_string_buffer(4096)                  # stands for the handles: a refused call looks at none of them
    h = C.addressof(handle)
    big, small_ = _VectorHead(None, 10, -1, b""), _VectorHead(None, 9, -1, b"")
    vec, short = C.addressof(big), C.addressof(small_)

    def jacobi(blas=h, sparse=h, r1=vec, w1=vec, w2=vec, dinv=vec, rule=_lib.RULE_CSHARP, shift=0.5):
        L.MgcgClearLastError()
        st = L.SolveMinresJacobi(blas, sparse, None, vec, vec, vec, vec, vec, vec, vec, vec, r1, w1, w2, dinv, 28, 10, shift, 1e-8, 0, 10, rule,
                                 C.byref(it), C.byref(res), C.byref(true), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    def vcycle(blas=h, sparse=h, mg=h, r1=vec, w1=vec, w2=vec, z=vec, rule=_lib.RULE_CSHARP, shift=0.5):
        L.MgcgClearLastError()
        st = L.SolveMinresMg(blas, sparse, None, mg, vec, vec, vec, vec, vec, vec, vec, vec, r1, w1, w2, z, 28, 10, shift, 1e-8, 0, 10, rule,
                             C.byref(it), C.byref(res), C.byref(true), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(r1=None), dict(w1=None), dict(w2=None), dict(dinv=None)):
        st, msg = jacobi(**kw)
        assert st == _lib.ERROR and "SolveMinresJacobi: null handle" in msg, (kw, msg)
    for kw in (dict(blas=None), dict(sparse=None), dict(mg=None), dict(r1=None), dict(w1=None), dict(w2=None), dict(z=None)):
        st, msg = vcycle(**kw)
        assert st == _lib.ERROR and "SolveMinresMg: null handle" in msg, (kw, msg)
    for call, who in ((jacobi, "SolveMinresJacobi"), (vcycle, "SolveMinresMg")):
        for shift in (float("nan"), float("inf"), -float("inf")):
            st, msg = call(shift=shift)
            assert st == _lib.ERROR and f"{who}: the shift is not finite" in msg, (shift, msg)
        st, msg = call(rule=_lib.RULE_HANDMADECL)
        assert st == _lib.ERROR and "max-norm" in msg and who in msg
        for rule in (-1, 5):
            st, msg = call(rule=rule)
            assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
        for name in ("r1", "w1", "w2"):
            st, msg = call(**{name: short})
            assert st == _lib.ERROR and f"{who}: the {name} vector holds 9 entries" in msg, (name, msg)
    st, msg = jacobi(dinv=short)
    assert st == _lib.ERROR and "the dinv vector holds 9 entries" in msg
    st, msg = vcycle(z=short)
    assert st == _lib.ERROR and "the z vector holds 9 entries" in msg
    # the several-ranks export, called without a communicator, refuses the same way
    L.MgcgClearLastError()
    st = L.SolveMinresJacobiParallel(None, h, h, None, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, vec, None, 10, 10, 0, 28, 0, 9, 0.5,
                                     1e-8, 0, 10, _lib.RULE_CSHARP, C.byref(it), C.byref(res), None, None, 0)
    assert st == _lib.ERROR and "SolveMinresJacobi: null handle" in _lib.last_error()
    L.MgcgClearLastError()
