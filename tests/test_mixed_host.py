"""Mixed-precision CG on the host side (no GPU needed): the yardstick of tests/test_gpu_mixed.py lives here and is checked for what
the method promises, the library exports the three entry points and refuses bad arguments before it asks for a device.

``mixed_cg_oracle`` is the loop of include/MgcgGpu.h (SolveMixed) in np.float32 / np.float64: every product goes into a named array
before the add that follows it, a row of either matrix is summed serially in stored order from +0.0, and every dot is a serial
left-to-right sum (np.add.accumulate adds one element after another).  Under dot_order = 1 the HIP loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems

FLT_MAX = 3.4028234663852886e38
UPDATE_EVERY = 4      # compiled into the library (kMixedUpdateEvery)
DROP = 0.01           # delta = 0.1, squared


# --------------------------------------------------------------------------- the yardstick
def stop_decision(rule, tol, min_it, max_it, it, rr_new, rr0):
    """The library's four 2-norm rules (decide_stop, include/MgcgGpu.h): (residual, shown in the trace, stop, status)."""
    res = math.sqrt(rr_new) if rr_new >= 0.0 else math.nan
    shown = res
    if rule == _lib.RULE_NATIVE:
        converged = min_it <= it and res < tol
    elif rule == _lib.RULE_SIMPLE:
        converged = min_it < it and res < tol
    elif rule == _lib.RULE_VIENNACL:
        shown = math.sqrt(rr_new / rr0) if rr_new / rr0 >= 0.0 else math.nan
        converged = min_it < it and rr_new / rr0 < tol * tol
    else:
        converged = min_it <= it <= max_it and res < tol
    status, stop = _lib.OK, converged
    if not stop and it >= min_it and it > max_it:
        stop, status = True, _lib.MAXIT_EXCEEDED
    if not stop and not math.isfinite(res):
        stop, status = True, _lib.NONFINITE
    return res, shown, stop, status


def serial_sum(terms):
    """((t0 + t1) + t2) + ... in the terms' own precision."""
    return float(np.add.accumulate(terms)[-1]) if len(terms) else 0.0


def row_sums(e, c, ro, x):
    """y_i = ((0 + e_k0 x_c0) + e_k1 x_c1) + ... in the dtype of e: every product rounded first, stored order."""
    n = len(ro) - 1
    prod = e * x[c]                                   # named array: rounded products
    y = np.zeros(n, dtype=e.dtype)
    length = np.diff(ro)
    for j in range(int(length.max()) if n else 0):
        rows = np.nonzero(length > j)[0]
        y[rows] = y[rows] + prod[ro[rows] + j]
    return y


def convert_elements(s):
    """(float)a for every stored value; ValueError naming the first row with a value that is not finite as a float."""
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e32 = e.astype(np.float32)
    bad = np.nonzero(~np.isfinite(e32))[0]
    if len(bad):
        rows = np.searchsorted(np.asarray(s.RowOffsets), bad, side="right") - 1
        raise ValueError(f"row {int(rows.min())} holds a value that is not finite as a float")
    return e32, bool((e32.astype(np.float64) == e).all())


def mixed_cg_oracle(s, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, x0=None):
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    e32, exact = convert_elements(s)
    x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x if x0 is None else x0, dtype=np.float64)
    r = b - row_sums(e, c, ro, x)
    rr0 = rr = maxrr = serial_sum(r * r)
    out = dict(exact=exact, updates=0, update_iterations=[], trace=[])
    if not math.sqrt(rr0) < FLT_MAX:
        out.update(x=x, r=r, iteration=0, residual=math.sqrt(rr0), status=_lib.NONFINITE, trace=np.array([]))
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = r.astype(np.float32)
    p32 = r32.copy()
    xs = np.zeros(s.Count, dtype=np.float32)
    want, it = False, 0
    while True:
        Ap32 = row_sums(e32, c, ro, p32)
        pAp = serial_sum(p32.astype(np.float64) * Ap32.astype(np.float64))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            alpha = rr / pAp if pAp != 0.0 else math.nan
            a32 = np.float32(alpha)
        if not (0.0 < pAp <= 1.79e308) or not np.isfinite(a32):          # breakdown: x keeps its last folded iterate, r the last true residual
            res = math.sqrt(rr)
            out["trace"].append(math.sqrt(rr / rr0) if rule == _lib.RULE_VIENNACL else res)
            status = _lib.NONFINITE
            break
        with np.errstate(over="ignore", invalid="ignore"):
            t = a32 * p32
            xs = xs + t
            u = (-a32) * Ap32
            r32 = r32 + u
            rn = serial_sum(r32.astype(np.float64) * r32.astype(np.float64))
        if rn > maxrr:
            maxrr = rn
        res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, it, rn, rr0)
        want = want or rn < DROP * maxrr or stop
        if it % UPDATE_EVERY == UPDATE_EVERY - 1 and want:
            x = x + xs.astype(np.float64)
            xs = np.zeros(s.Count, dtype=np.float32)
            r = b - row_sums(e, c, ro, x)
            rn = serial_sum(r * r)
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, it, rn, rr0)
            if not stop and not res < FLT_MAX:
                stop, status = True, _lib.NONFINITE
            with np.errstate(over="ignore", invalid="ignore"):
                r32 = r.astype(np.float32)
            maxrr = rn
            want = False
            out["updates"] += 1
            out["update_iterations"].append(it)
            out["trace"].append(shown)
            if stop:
                break
        else:
            out["trace"].append(shown)
        with np.errstate(over="ignore", invalid="ignore"):
            beta = rn / rr
            b32 = np.float32(beta)
            v = b32 * p32
            p32 = r32 + v
        rr = rn
        it += 1
    out.update(x=x, r=r, iteration=it, residual=res, status=status, trace=np.array(out["trace"]))
    return out


# --------------------------------------------------------------------------- what it is measured against
def _product(s, v):
    """A v in fp64, any summation order (the independent residual and the plain loop below)."""
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    return np.bincount(rows, weights=s.Elements[: s.nnz] * v[s.ColumnIndeces[: s.nnz]], minlength=s.Count)


def true_relative_residual(s, x):
    return float(np.linalg.norm(s.b - _product(s, x)) / np.linalg.norm(s.b))


def plain_cg_iterations(s, rel):
    """Textbook float64 CG from x = 0 to || r || < rel || b || on the recurrence's residual: loop bodies run."""
    b = np.asarray(s.b, dtype=np.float64)
    x, r = np.zeros(s.Count), b.copy()
    p, rr = r.copy(), float(r @ r)
    goal = rel * math.sqrt(rr)
    for it in range(5000):
        Ap = _product(s, p)
        alpha = rr / float(p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        rn = float(r @ r)
        if math.sqrt(rn) < goal:
            return it + 1
        p = r + (rn / rr) * p
        rr = rn
    raise AssertionError("the plain loop did not converge")


def poisson16_random():
    s = problems.poisson(16, 16, 16)
    b = np.random.default_rng(20261018).standard_normal(s.Count)
    return problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count), b, "poisson16-randn", s.grid)


SYSTEMS = {"poisson16": poisson16_random, "viennacl4000": lambda: problems.viennacl_main(4000)}
_cache = {}


def _solved(name, rel):
    if (name, rel) not in _cache:
        s = SYSTEMS[name]()
        tol = rel * float(np.linalg.norm(s.b))
        _cache[(name, rel)] = (s, mixed_cg_oracle(s, rule=_lib.RULE_CSHARP, tol=tol, max_it=2000), plain_cg_iterations(s, rel))
    return _cache[(name, rel)]


@pytest.mark.parametrize("rel", [1e-8, 1e-12])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_the_yardstick_reaches_fp64_accuracy_in_fp64_s_iteration_count(name, rel):
    s, o, plain = _solved(name, rel)
    assert o["status"] == _lib.OK
    achieved = true_relative_residual(s, o["x"])
    mixed = o["iteration"] + 1
    print(f"{name} rel {rel:g}: true residual {achieved:.3e}, mixed {mixed} iterations, fp64 CG {plain}, {o['updates']} reliable updates")
    assert achieved < rel
    assert mixed <= 1.25 * plain
    # the reported residual is the true one: sqrt(r.r) of the r that came back
    assert o["residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_updates_happen_only_in_every_fourth_iteration(name):
    _, o, _ = _solved(name, 1e-12)
    assert o["updates"] == len(o["update_iterations"]) >= 2
    assert all(it % 4 == 3 for it in o["update_iterations"])
    assert o["update_iterations"][-1] == o["iteration"]              # the stop is decided in an update, and only there
    assert len(o["trace"]) == o["iteration"] + 1


def test_a_value_beyond_the_float_range_is_refused():
    s = problems.poisson(4, 4, 4)
    e = s.Elements.copy()
    k = int(s.RowOffsets[37]) + 2
    e[k] = 1e39
    bad = problems.LinearSystem(e, s.ColumnIndeces, s.RowOffsets, s.x, s.b, "poisson4-1e39", s.grid)
    with pytest.raises(ValueError, match="row 37 "):
        mixed_cg_oracle(bad)
    with pytest.raises(ValueError, match="row 37 "):
        convert_elements(bad)


def test_an_inexact_matrix_still_converges_to_1e_12():
    """The sin-band driver matrix has values that are no fp32 numbers: the inner loop solves a perturbed system, the updates see the true one."""
    s, o, _ = _solved("viennacl4000", 1e-12)
    assert o["exact"] is False
    assert convert_elements(problems.poisson(5, 5, 5))[1] is True
    assert o["status"] == _lib.OK and true_relative_residual(s, o["x"]) < 1e-12


def test_row_sums_are_serial_in_stored_order():
    """Three entries whose float sum depends on the order: (1e8 + 1) - 1e8 = 0 in float, (1e8 - 1e8) + 1 = 1."""
    ro = np.array([0, 3, 6], dtype=np.int32)
    c = np.array([0, 1, 2, 0, 2, 1], dtype=np.int32)
    e = np.array([1e8, 1.0, -1e8, 1e8, -1e8, 1.0], dtype=np.float32)
    y = row_sums(e, c, ro, np.ones(3, dtype=np.float32))
    assert y.dtype == np.float32 and y.tolist() == [0.0, 1.0]
    assert serial_sum(np.array([1e16, 1.0, -1e16])) == 0.0 and serial_sum(np.array([1e16, -1e16, 1.0])) == 1.0


# --------------------------------------------------------------------------- the library's host side
def test_the_three_symbols_are_exported_and_bound(hiplib):
    for name in ("MgcgMixedSetup", "CsrMVFloat", "SolveMixed"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import mixed

    assert "mixed" in conjugategradient_amd.__all__ and "``mixed``" in conjugategradient_amd.__doc__
    assert issubclass(mixed.ConjugateGradientMixedGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    cg = mixed.ConjugateGradientMixedGpu.__new__(mixed.ConjugateGradientMixedGpu)
    cg._ready = False
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    L.MgcgClearLastError()
    assert L.MgcgMixedSetup(None, None, None, None, 10, 5, None, None) == -1
    assert "MgcgMixedSetup: null handle" in _lib.last_error()
    L.MgcgClearLastError()
    it, res, up = C.c_int(0), C.c_double(0.0), C.c_int(0)
    args = (10, 5, 1e-8, 0, 10)
    st = L.SolveMixed(None, None, None, None, None, None, None, None, None, None, None, None, *args, _lib.RULE_NATIVE,
                      C.byref(it), C.byref(res), C.byref(up), None, 0)
    assert st == _lib.ERROR and "SolveMixed: null handle" in _lib.last_error()
    L.MgcgClearLastError()
