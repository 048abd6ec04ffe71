"""Single-reduction CG on the host side (no GPU needed): the yardstick of tests/test_gpu_sreduce.py lives here and is checked against
classical CG, the library exports the two entry points and refuses bad arguments before it asks for a device.

``sreduce_cg_oracle`` is the loop of include/MgcgGpu.h (SolveSingleReduce) in np.float64: every product goes into a named array before
the add that follows it, a matrix row is summed serially in stored order from +0.0 (``row_sums``), the scalars are evaluated in the
header's order, and every sum is a serial left-to-right sum (``serial_sum``), cut at ``parts`` and added in rank order.  Under
dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums, serial_sum

DBL_BIG = 1.79e308


# --------------------------------------------------------------------------- the yardstick
def stop_decision(rule, tol, min_it, max_it, it, rr_new, rr0):
    """The library's four 2-norm rules (decide_stop, include/MgcgGpu.h): (residual, shown in the trace, stop, status)."""
    with np.errstate(all="ignore"):
        rr_new, rr0 = np.float64(rr_new), np.float64(rr0)
        res = float(np.sqrt(rr_new))
        shown = res
        if rule == _lib.RULE_NATIVE:
            converged = min_it <= it and res < tol
        elif rule == _lib.RULE_SIMPLE:
            converged = min_it < it and res < tol
        elif rule == _lib.RULE_VIENNACL:
            shown = float(np.sqrt(rr_new / rr0))
            converged = min_it < it and bool(rr_new / rr0 < tol * tol)
        else:
            converged = min_it <= it <= max_it and res < tol
    status, stop = _lib.OK, converged
    if not stop and it >= min_it and it > max_it:
        stop, status = True, _lib.MAXIT_EXCEEDED
    if not stop and not math.isfinite(res):
        stop, status = True, _lib.NONFINITE
    return res, shown, stop, status


def diagonal_of(s):
    """a_ii = the first stored entry of row i whose column is i."""
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    k = np.nonzero(np.asarray(s.ColumnIndeces[: s.nnz]) == rows)[0][::-1]       # reversed: the first stored entry is assigned last
    d = np.zeros(s.Count)
    d[rows[k]] = np.asarray(s.Elements)[k]
    return d


def sreduce_cg_oracle(s, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, jacobi=False, parts=None, x0=None, diag=None, total=serial_sum):
    """total(terms): the sum of one rank's terms (default: serial, left to right)."""
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    parts = [0, s.Count] if parts is None else [int(v) for v in parts]
    dinv = 1.0 / (diagonal_of(s) if diag is None else diag) if jacobi else None

    def sums(terms):
        acc = 0.0
        for lo, hi in zip(parts[:-1], parts[1:]):
            acc += total(terms[lo:hi]) if hi > lo else 0.0
        return acc

    def precondition(r):
        return dinv * r if jacobi else r

    x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
    r = b - row_sums(e, c, ro, x)
    u = precondition(r)
    rr0 = rr = sums(r * r)
    gamma = sums(r * u) if jacobi else rr
    w = row_sums(e, c, ro, u)
    delta = sums(w * u)
    p = sv = None
    gamma_old = alpha_old = 0.0
    trace, k = [], 0
    with np.errstate(all="ignore"):
        res = float(np.sqrt(np.float64(rr)))
        shown = float(np.sqrt(np.float64(rr) / np.float64(rr0))) if rule == _lib.RULE_VIENNACL else res
    while True:
        if k > 0:                                        # body k - 1's stop decision, behind the product of body k
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k - 1, rr, rr0)
            trace.append(shown)
            if stop:
                it = k - 1
                break
        with np.errstate(all="ignore"):
            g = np.float64(gamma)
            beta, den = np.float64(0.0), np.float64(delta)
            if k > 0:
                beta = g / np.float64(gamma_old)
                t = beta * g
                q = t / np.float64(alpha_old)
                den = np.float64(delta) - q
            alpha = g / den
        if not (0.0 < den <= DBL_BIG) or not (abs(alpha) <= DBL_BIG):      # breakdown, before this body's updates
            trace.append(shown)
            it, status = k, _lib.NONFINITE
            break
        beta, alpha = float(beta), float(alpha)
        if k == 0:
            p, sv = u.copy(), w.copy()
        else:
            bp = beta * p
            p = u + bp
            bs = beta * sv
            sv = w + bs
        ap = alpha * p
        x = x + ap
        as_ = (-alpha) * sv
        r = r + as_
        u = precondition(r)
        gamma_old, alpha_old = gamma, alpha
        rr = sums(r * r)
        gamma = sums(r * u) if jacobi else rr
        w = row_sums(e, c, ro, u)
        delta = sums(w * u)
        k += 1
    return dict(x=x, r=r, iteration=it, residual=res, status=status, trace=np.array(trace))


# --------------------------------------------------------------------------- what it is measured against
def tridiagonal(n):
    """Symmetric tridiagonal, -1 off the diagonal, the diagonal 2.5 + (i mod 7) (strictly dominant), b = cos(0.3 i).  Returns (system, diagonal)."""
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    diag = 2.5 + (i % 7)
    vals = np.stack([-np.ones(n), diag, -np.ones(n)], axis=1)
    keep = (cols >= 0) & (cols < n)
    ro = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return problems.LinearSystem(vals[keep], cols[keep].astype(np.int32), ro, np.zeros(n), np.cos(0.3 * i), "tridiagonal"), diag


def with_b(s, b, name):
    return problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count), b, name, s.grid)


def randn_b(s, name):
    return with_b(s, np.random.default_rng(20261018).standard_normal(s.Count), name + "-randn")


def _product(s, v):
    """A v in fp64, any summation order (the independent residual and the classical loop below)."""
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * v[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


def true_relative_residual(s, x):
    return float(np.linalg.norm(s.b - _product(s, x)) / np.linalg.norm(s.b))


def classical_cg_iteration(s, goal, dinv=None):
    """Textbook float64 (P)CG from x = 0 with numpy's own dots: the index of the first body whose recurrence residual has || r || < goal."""
    b = np.asarray(s.b, dtype=np.float64)
    r = b.copy()
    z = r if dinv is None else dinv * r
    p, rz = z.copy(), float(r @ z)
    for it in range(20000):
        Ap = _product(s, p)
        alpha = rz / float(p @ Ap)
        r = r - alpha * Ap
        if math.sqrt(float(r @ r)) < goal:
            return it
        z = r if dinv is None else dinv * r
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise AssertionError("the classical loop did not converge")


SYSTEMS = {
    "poisson16": lambda: randn_b(problems.poisson(16, 16, 16), "poisson16"),
    "poisson32x32": lambda: randn_b(problems.poisson(32, 32), "poisson32x32"),
    "viennacl4000": lambda: randn_b(problems.viennacl_main(4000), "viennacl4000"),
    "random_spd5000": lambda: randn_b(problems.random_spd(5000), "random_spd5000"),
}
_systems = {}


def system(name):
    if name not in _systems:
        s = SYSTEMS[name]()
        _systems[name] = (s, diagonal_of(s))
    return _systems[name]


@pytest.mark.parametrize("rel", [1e-8, 1e-12])
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_the_yardstick_stops_within_one_iteration_of_classical_cg(name, jacobi, rel):
    s, diag = system(name)
    goal = rel * float(np.linalg.norm(s.b))
    o = sreduce_cg_oracle(s, rule=_lib.RULE_CSHARP, tol=goal, max_it=20000, jacobi=jacobi, diag=diag)
    classical = classical_cg_iteration(s, goal, 1.0 / diag if jacobi else None)
    achieved = true_relative_residual(s, o["x"])
    print(f"{name} jacobi={jacobi} rel {rel:g}: single-reduction stops in body {o['iteration']}, classical CG in {classical}, true residual {achieved:.3e}")
    assert o["status"] == _lib.OK
    assert abs(o["iteration"] - classical) <= 1
    assert achieved < rel
    assert len(o["trace"]) == o["iteration"] + 1
    # the residual that came back is the one that was judged
    assert o["residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_serial_yardstick(rule):
    s, diag = system("poisson32x32")
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else 1e-8 * float(np.linalg.norm(s.b))
    o = sreduce_cg_oracle(start, rule=rule, tol=tol, max_it=2000)
    assert o["status"] == _lib.OK and o["iteration"] >= 10
    zero = sreduce_cg_oracle(s, rule=rule, tol=tol, max_it=2000)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert (o["iteration"] == zero["iteration"] and np.array_equal(o["x"], zero["x"])) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2]
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]


def test_the_iteration_cap_and_the_minimum_are_kept():
    s, diag = system("poisson16")
    capped = sreduce_cg_oracle(s, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    free = sreduce_cg_oracle(s, tol=1e-2 * float(np.linalg.norm(s.b)), max_it=400)
    held = sreduce_cg_oracle(s, tol=1e-2 * float(np.linalg.norm(s.b)), min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5


def test_breakdowns_are_reported_as_nonfinite():
    ro = np.array([0, 2, 4], dtype=np.int32)
    c = np.array([0, 1, 0, 1], dtype=np.int32)
    indefinite = problems.LinearSystem(np.array([1.0, 2.0, 2.0, 1.0]), c, ro, np.array([0.25, -0.5]), np.array([1.0, -1.0]), "indefinite2")
    for jacobi in (False, True):
        o = sreduce_cg_oracle(indefinite, tol=1e-12, jacobi=jacobi)
        assert o["status"] == _lib.NONFINITE and o["iteration"] == 0, o       # r0 = (1.75, -1): u.Au < 0 in body 0
        assert np.array_equal(o["x"], indefinite.x) and len(o["trace"]) == 1
    s, _ = tridiagonal(50)
    zero = sreduce_cg_oracle(with_b(s, np.zeros(50), "b0"), tol=1e-12)
    assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
    zero = sreduce_cg_oracle(with_b(s, np.zeros(50), "b0"), rule=_lib.RULE_VIENNACL, tol=1e-12)
    assert zero["status"] == _lib.NONFINITE and math.isnan(zero["trace"][0])


def test_sums_are_cut_at_the_ranks_and_added_in_rank_order():
    s, diag = system("viennacl4000")
    one = sreduce_cg_oracle(s, tol=1e-6, jacobi=True, diag=diag)
    cut = sreduce_cg_oracle(s, tol=1e-6, jacobi=True, diag=diag, parts=problems.partition_offsets(s.Count, 4))
    assert abs(one["iteration"] - cut["iteration"]) <= 1 and not np.array_equal(one["x"], cut["x"])
    assert np.abs(one["x"] - cut["x"]).max() <= 1e-10 * np.abs(one["x"]).max()
    empty = sreduce_cg_oracle(s, tol=1e-6, jacobi=True, diag=diag, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- the library's host side
def test_the_two_symbols_are_exported_and_bound(hiplib):
    for name in ("SolveSingleReduce", "SolveSingleReduceParallel"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import singlereduce

    assert "singlereduce" in conjugategradient_amd.__all__ and "``singlereduce``" in conjugategradient_amd.__doc__
    assert issubclass(singlereduce.ConjugateGradientSingleReduceGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    cg = singlereduce.ConjugateGradientSingleReduceGpu.__new__(singlereduce.ConjugateGradientSingleReduceGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    with pytest.raises(ValueError, match="max-norm"):
        singlereduce.ConjugateGradientSingleReduceGpu(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    it, res = C.c_int(0), C.c_double(0.0)
    handle = C.create_string_buffer(4096)                  # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    big, small = _VectorHead(None, 10, -1, b""), _VectorHead(None, 9, -1, b"")
    vec = C.addressof(big)

    def call(blas=h, sparse=h, s=vec, dinv=None, rule=_lib.RULE_CSHARP):
        L.MgcgClearLastError()
        st = L.SolveSingleReduce(blas, sparse, None, vec, vec, vec, vec, vec, vec, vec, vec, s, dinv, 28, 10, 1e-8, 0, 10, rule,
                                 C.byref(it), C.byref(res), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(s=None)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "SolveSingleReduce: null handle" in msg, (kw, msg)
    st, msg = call(rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "SolveSingleReduce" in msg
    for rule in (-1, 5):
        st, msg = call(rule=rule)
        assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
    st, msg = call(s=C.addressof(small))
    assert st == _lib.ERROR and "the s vector holds 9 entries" in msg
    st, msg = call(dinv=C.addressof(small))
    assert st == _lib.ERROR and "the dinv vector holds 9 entries" in msg
    # the several-ranks export, called without a communicator, refuses the same way
    L.MgcgClearLastError()
    st = L.SolveSingleReduceParallel(None, h, h, None, vec, vec, vec, vec, vec, vec, vec, vec, vec, None, 10, 10, 0, 28, 0, 9,
                                     1e-8, 0, 10, _lib.RULE_HANDMADECL, C.byref(it), C.byref(res), None, 0)
    assert st == _lib.ERROR and "max-norm" in _lib.last_error()
    L.MgcgClearLastError()
