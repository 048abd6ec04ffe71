"""Chebyshev-preconditioned CG on the host side (no GPU needed): the yardstick of tests/test_gpu_chebyshev.py lives here and is checked
against the polynomial's closed form, against classical CG and against the Jacobi yardstick; the library exports the three entry points
and refuses bad arguments before it asks for a device.

``chebyshev_cg_oracle`` is the loop of include/MgcgGpu.h (SolveChebyshev) in np.float64: the coefficients in the header's order, every
product in a named array before the add that follows it, a matrix row summed serially in stored order from +0.0 (``row_sums``), every
sum a serial left-to-right sum (``serial_sum``) cut at ``parts`` and added in rank order.  Under dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums, serial_sum
from tests.test_sreduce_host import classical_cg_iteration, diagonal_of, randn_b, stop_decision, tridiagonal, true_relative_residual

DBL_BIG = 1.79e308


# --------------------------------------------------------------------------- the yardstick
def chebyshev_coefficients(m, lmin, lmax):
    """(it, c1[1 .. m-1], c2[1 .. m-1]) in the header's order of operations; Python floats are IEEE doubles."""
    theta = (lmax + lmin) * 0.5
    delta = (lmax - lmin) * 0.5
    sigma = theta / delta
    rho = 1.0 / sigma
    it = 1.0 / theta
    c1, c2 = [None], [None]
    for _ in range(1, m):
        nxt = 1.0 / (2.0 * sigma - rho)
        c1.append(nxt * rho)
        c2.append((2.0 * nxt) / delta)
        rho = nxt
    return it, c1, c2


def chebyshev_apply(e, c, ro, r, dinv, m, lmin, lmax):
    """z = M r: the first pass and m - 1 steps."""
    it, c1, c2 = chebyshev_coefficients(m, lmin, lmax)
    u = dinv * r if dinv is not None else r
    d = it * u
    z = d.copy()
    for j in range(1, m):
        acc = row_sums(e, c, ro, z)
        res = r - acc
        t = dinv * res if dinv is not None else res
        a = c1[j] * d
        b = c2[j] * t
        d = a + b
        z = z + d
    return z


def positive(v):
    return bool(0.0 < v <= DBL_BIG)


def gershgorin_oracle(s, dinv=None, lo=0, hi=None):
    """max over rows [lo, hi) of sum_j |a_ij| (times dinv_i), each row summed in stored order from +0.0; 0 for an empty slice."""
    hi = s.Count if hi is None else hi
    if hi <= lo:
        return 0.0
    e = np.abs(np.asarray(s.Elements[: s.nnz], dtype=np.float64))
    sums = row_sums(e, np.zeros(s.nnz, dtype=np.int64), np.asarray(s.RowOffsets), np.ones(1))
    if dinv is not None:
        sums = dinv * sums
    return float(sums[lo:hi].max())


def chebyshev_cg_oracle(s, degree, bounds, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, jacobi=False, parts=None, x0=None, diag=None,
                        total=serial_sum):
    """total(terms): the sum of one rank's terms (default: serial, left to right).  The dict also carries ``first_rz``."""
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    parts = [0, s.Count] if parts is None else [int(v) for v in parts]
    dinv = 1.0 / (diagonal_of(s) if diag is None else diag) if jacobi else None
    lmin, lmax = bounds

    def sums(terms):
        acc = 0.0
        for lo, hi in zip(parts[:-1], parts[1:]):
            acc += total(terms[lo:hi]) if hi > lo else 0.0
        return acc

    def shown_of(rr, rr0):
        with np.errstate(all="ignore"):
            res = float(np.sqrt(np.float64(rr)))
            return res, (float(np.sqrt(np.float64(rr) / np.float64(rr0))) if rule == _lib.RULE_VIENNACL else res)

    x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
    r = b - row_sums(e, c, ro, x)
    z = chebyshev_apply(e, c, ro, r, dinv, degree, lmin, lmax)
    rr0 = rr = sums(r * r)
    rz = first_rz = sums(r * z)
    trace, it = [], 0
    res, shown = shown_of(rr, rr0)
    if not positive(rz):                                   # an indefinite polynomial, or r = 0: iteration 0 cannot run
        return dict(x=x, r=r, iteration=0, residual=res, status=_lib.NONFINITE, trace=np.array([shown]), first_rz=first_rz)
    p = z.copy()
    while True:
        Ap = row_sums(e, c, ro, p)
        pAp = sums(p * Ap)
        if not positive(pAp):                              # before this iteration's updates: the last judged residual once more
            trace.append(shown)
            status = _lib.NONFINITE
            break
        with np.errstate(all="ignore"):
            alpha = float(np.float64(rz) / np.float64(pAp))
        u = (-alpha) * Ap
        r = r + u
        rr = sums(r * r)
        z = chebyshev_apply(e, c, ro, r, dinv, degree, lmin, lmax)
        rz_new = sums(r * z)
        res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, it, rr, rr0)
        trace.append(shown)
        ap = alpha * p
        x = x + ap                                         # the iteration is complete either way
        if stop:
            break
        if not positive(rz_new):                           # the NEXT iteration cannot start
            it += 1
            trace.append(shown)
            status = _lib.NONFINITE
            break
        with np.errstate(all="ignore"):
            beta = float(np.float64(rz_new) / np.float64(rz))
        bp = beta * p
        p = z + bp
        rz = rz_new
        it += 1
    return dict(x=x, r=r, iteration=it, residual=res, status=status, trace=np.array(trace), first_rz=first_rz)


# --------------------------------------------------------------------------- (a) the polynomial against its closed form
def _dense_spd(n=12, seed=3):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, n))
    A = q @ q.T + n * np.eye(n)
    ro = np.arange(0, n * n + 1, n, dtype=np.int32)
    c = np.tile(np.arange(n, dtype=np.int32), n)
    return A, problems.LinearSystem(A.reshape(-1).copy(), c, ro, np.zeros(n), rng.standard_normal(n), "dense-spd12")


def _chebyshev_T(m, X):
    """T_m(X) for a matrix or a scalar by the three-term recurrence."""
    one = np.eye(len(X)) if np.ndim(X) == 2 else 1.0
    t0, t1 = one, X
    if m == 0:
        return t0
    for _ in range(m - 1):
        t0, t1 = t1, 2.0 * (X @ t1 if np.ndim(X) == 2 else X * t1) - t0
    return t1


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("m", range(1, 9))
def test_the_recurrence_is_the_chebyshev_polynomial(m, jacobi):
    A, s = _dense_spd()
    n = s.Count
    dinv = 1.0 / np.diag(A) if jacobi else None
    B = A * dinv[:, None] if jacobi else A
    ev = np.linalg.eigvals(B).real
    lmin, lmax = 0.9 * ev.min(), 1.1 * ev.max()
    r = np.asarray(s.b)
    z = chebyshev_apply(np.asarray(s.Elements), np.asarray(s.ColumnIndeces), np.asarray(s.RowOffsets), r, dinv, m, lmin, lmax)
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    u = dinv * r if jacobi else r
    closed = (np.eye(n) - _chebyshev_T(m, (theta * np.eye(n) - B) / delta) / _chebyshev_T(m, theta / delta)) @ np.linalg.solve(B, u)
    err = float(np.linalg.norm(z - closed) / np.linalg.norm(closed))
    print(f"m = {m} jacobi = {jacobi}: relative distance to the closed form {err:.2e}")
    assert err <= 1e-10


# --------------------------------------------------------------------------- (b) iteration counts
_poisson = {}


def poisson16():
    if not _poisson:
        s = randn_b(problems.poisson(16, 16, 16), "poisson16")
        _poisson["s"] = (s, diagonal_of(s))
    return _poisson["s"]


def default_bounds(s, dinv=None, ratio=30.0):
    lmax = gershgorin_oracle(s, dinv)
    return lmax / ratio, lmax


def test_iteration_counts_fall_with_the_degree():
    s, diag = poisson16()
    goal = 1e-8 * float(np.linalg.norm(s.b))
    bounds = default_bounds(s)
    assert bounds[1] == 12.0
    plain = classical_cg_iteration(s, goal) + 1              # loop bodies
    counts = []
    for m in (1, 2, 4, 8):
        o = chebyshev_cg_oracle(s, m, bounds, tol=goal, max_it=400, diag=diag)
        achieved = true_relative_residual(s, o["x"])
        print(f"16^3 Poisson, m = {m}: {o['iteration'] + 1} bodies (plain CG {plain}), true relative residual {achieved:.3e}")
        assert o["status"] == _lib.OK and achieved < 1e-8
        assert len(o["trace"]) == o["iteration"] + 1 and o["residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))
        counts.append(o["iteration"] + 1)
    assert all(a > b for a, b in zip(counts[:-1], counts[1:])), counts
    assert abs(counts[0] - plain) <= 1, (counts, plain)


# --------------------------------------------------------------------------- (c) the Jacobi anchor
@pytest.mark.parametrize("parts", [None, [0, 100, 100, 300]])
def test_degree_one_with_theta_one_is_the_jacobi_yardstick(parts):
    from tests.test_gpu_jacobi import jacobi_pcg_oracle

    s, diag = tridiagonal(300)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    e, c, ro = np.asarray(s.Elements[: s.nnz]), np.asarray(s.ColumnIndeces[: s.nnz]), np.asarray(s.RowOffsets)

    def set_added(left, right, a):
        t = a * right
        return left + t

    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        t = 1e-8 if rule == _lib.RULE_VIENNACL else tol
        ref = jacobi_pcg_oracle(s, rule, t, parts=parts, diag=diag, dot=lambda a, b: serial_sum(a * b), spmv=lambda v: row_sums(e, c, ro, v), set_added=set_added)
        got = chebyshev_cg_oracle(s, 1, (0.5, 1.5), rule, t, jacobi=True, diag=diag, parts=parts)
        assert ref["status"] == got["status"] == _lib.OK and ref["iteration"] == got["iteration"] >= 5
        assert ref["residual"] == got["residual"] and np.array_equal(ref["trace"], got["trace"]) and np.array_equal(ref["x"], got["x"])


# --------------------------------------------------------------------------- (d) an indefinite preconditioner
def test_an_upper_bound_below_the_spectrum_shows_as_a_negative_rz():
    s, diag = tridiagonal(300)
    lmax = gershgorin_oracle(s) / 4.0
    o = chebyshev_cg_oracle(s, 2, (lmax / 30.0, lmax), tol=1e-8)
    print("first r.z", o["first_rz"])
    assert o["first_rz"] < 0.0
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 0 and np.array_equal(o["x"], s.x) and len(o["trace"]) == 1
    assert o["residual"] == math.sqrt(serial_sum(np.asarray(s.b) ** 2))
    # b = 0: r.z = 0
    zero = problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(300), np.zeros(300), "b0")
    o = chebyshev_cg_oracle(zero, 3, default_bounds(s), tol=1e-8)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 0 and o["residual"] == 0.0 and not o["x"].any()


def test_the_gershgorin_oracle_bounds_the_spectrum():
    A, s = _dense_spd()
    assert gershgorin_oracle(s) >= np.linalg.eigvalsh(A).max()
    assert gershgorin_oracle(s) == max(serial_sum(np.abs(row)) for row in A)
    dinv = 1.0 / np.diag(A)
    assert gershgorin_oracle(s, dinv) >= np.linalg.eigvals(A * dinv[:, None]).real.max()
    assert gershgorin_oracle(s, None, 5, 5) == 0.0 and gershgorin_oracle(s, None, 3, 4) == serial_sum(np.abs(A[3]))


def test_sums_are_cut_at_the_ranks_and_added_in_rank_order():
    s, diag = poisson16()
    goal = 1e-8 * float(np.linalg.norm(s.b))
    one = chebyshev_cg_oracle(s, 3, default_bounds(s), tol=goal)
    cut = chebyshev_cg_oracle(s, 3, default_bounds(s), tol=goal, parts=problems.partition_offsets(s.Count, 4))
    assert abs(one["iteration"] - cut["iteration"]) <= 1 and not np.array_equal(one["x"], cut["x"])
    assert np.abs(one["x"] - cut["x"]).max() <= 1e-10 * np.abs(one["x"]).max()
    empty = chebyshev_cg_oracle(s, 3, default_bounds(s), tol=goal, parts=[0, 0, s.Count])
    assert np.array_equal(empty["x"], one["x"]) and np.array_equal(empty["trace"], one["trace"])


# --------------------------------------------------------------------------- (e) the library's host side
def test_the_three_symbols_are_exported_and_bound(hiplib):
    for name in ("MgcgGershgorinBound", "SolveChebyshev", "SolveChebyshevParallel"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import chebyshev, parallel

    assert "chebyshev" in conjugategradient_amd.__all__ and "``chebyshev``" in conjugategradient_amd.__doc__
    assert issubclass(chebyshev.ConjugateGradientChebyshevGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    assert callable(parallel.ConjugateGradientRankGpu.SolveChebyshev)
    cg = chebyshev.ConjugateGradientChebyshevGpu.__new__(chebyshev.ConjugateGradientChebyshevGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    with pytest.raises(ValueError, match="max-norm"):
        chebyshev.ConjugateGradientChebyshevGpu(10, 3, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)
    for kw in (dict(degree=0), dict(degree=17), dict(bounds=(0.0, 1.0)), dict(bounds=(2.0, 1.0)), dict(bounds=(1.0, math.inf)), dict(eigRatio=1.0)):
        with pytest.raises(ValueError):
            chebyshev.ConjugateGradientChebyshevGpu(10, 3, 0, 10, 1e-8, **kw)


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
    nan = float("nan")

    def call(blas=h, sparse=h, dinv=None, z=vec, z2=vec, d=vec, degree=4, lmin=0.4, lmax=12.0, rule=_lib.RULE_CSHARP):
        L.MgcgClearLastError()
        st = L.SolveChebyshev(blas, sparse, None, vec, vec, vec, vec, vec, vec, vec, vec, dinv, z, z2, d, 28, 10, degree, lmin, lmax,
                              1e-8, 0, 10, rule, C.byref(it), C.byref(res), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(z=None), dict(z2=None), dict(d=None)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "SolveChebyshev: null handle" in msg, (kw, msg)
    for degree in (0, -1, 17):
        st, msg = call(degree=degree)
        assert st == _lib.ERROR and f"degree {degree}, must be 1 .. 16" in msg
    for lmin, lmax in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (nan, 1.0), (1.0, nan), (1.0, math.inf)):
        st, msg = call(lmin=lmin, lmax=lmax)
        assert st == _lib.ERROR and "0 < lambdaMin < lambdaMax" in msg, (lmin, lmax, msg)
    st, msg = call(rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "SolveChebyshev" in msg
    for rule in (-1, 5):
        st, msg = call(rule=rule)
        assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
    for kw, word in ((dict(z=C.addressof(small)), "the z vector holds 9"), (dict(z2=C.addressof(small)), "the z2 vector holds 9"),
                     (dict(d=C.addressof(small)), "the d vector holds 9"), (dict(dinv=C.addressof(small)), "the dinv vector holds 9")):
        st, msg = call(**kw)
        assert st == _lib.ERROR and word in msg, (kw, msg)
    # the several-ranks export, called without a communicator, refuses the same way
    L.MgcgClearLastError()
    st = L.SolveChebyshevParallel(None, h, h, None, vec, vec, vec, vec, vec, vec, vec, vec, None, vec, vec, vec, 10, 10, 0, 28, 0, 9, 17, 0.4, 12.0,
                                  1e-8, 0, 10, _lib.RULE_CSHARP, C.byref(it), C.byref(res), None, 0)
    assert st == _lib.ERROR and "degree 17" in _lib.last_error()
    L.MgcgClearLastError()
    # the bound: null handles and a dinv vector that is too small
    bound = C.c_double(-1.0)
    assert L.MgcgGershgorinBound(None, vec, vec, vec, 28, 10, 0, None, C.byref(bound)) == -1 and "MgcgGershgorinBound: null handle" in _lib.last_error()
    L.MgcgClearLastError()
    assert L.MgcgGershgorinBound(h, vec, vec, vec, 28, 10, 0, None, None) == -1 and "null handle" in _lib.last_error()
    L.MgcgClearLastError()
    wide = _VectorHead(None, 28, -1, b"")
    assert L.MgcgGershgorinBound(h, C.addressof(wide), C.addressof(wide), C.addressof(wide), 28, 10, 0, C.addressof(small), C.byref(bound)) == -1
    assert "the dinv vector holds 9 entries" in _lib.last_error()
    L.MgcgClearLastError()
    # an empty local slice needs no device: the bound is 0
    assert L.MgcgGershgorinBound(h, C.addressof(wide), C.addressof(wide), C.addressof(wide), 0, 0, 0, None, C.byref(bound)) == 0 and bound.value == 0.0
