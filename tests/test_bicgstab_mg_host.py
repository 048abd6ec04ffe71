"""V-cycle-preconditioned BiCGStab on the host side (no GPU needed): the yardstick of tests/test_gpu_bicgstab_mg.py lives here and is
checked against ``bicgstab_oracle``, against the true residual and on the corner cases of the method; the library exports the entry point
and refuses bad arguments before it asks for a device.

``pbicgstab_oracle`` is ``bicgstab_oracle`` (tests/test_bicgstab_host.py) restated with a callable M^-1 and the same rounding order: the
loop of include/MgcgGpu.h (SolveBicgstabMg) in np.float64 with phat = minv(p) and shat = minv(s).  The V-cycle is ``Hierarchy.apply``
(tests/test_amg_host.py), built from the matrix itself ("own") or from its symmetric part ("sym"), with the 2x2x2 box maps of the geometric
set-up ("box": 3 levels, the class's omega) or by the matching with the aggregation class's defaults ("agg").  Under dot_order = 1 the HIP
loop must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import Hierarchy, box_maps, csr_of
from tests.test_bicgstab_host import DBL_BIG, MAX_IT, SEED, bicgstab_oracle, numpy_true_residual, rho_zero2, sigma_zero2
from tests.test_bicgstab_host import _product, system as bicgstab_system
from tests.test_mixed_host import row_sums
from tests.test_sreduce_host import diagonal_of, serial_sum, stop_decision, with_b


# --------------------------------------------------------------------------- the yardstick
def pbicgstab_oracle(s, minv, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, x0=None, total=serial_sum):
    """A x = s.b from s.x (x0), right-preconditioned with the fixed linear map minv(v) = M^-1 v.  One rank; total(terms): the sum of the
    terms (default: serial, left to right)."""
    e = np.asarray(s.Elements[: s.nnz], dtype=np.float64)
    c = np.asarray(s.ColumnIndeces[: s.nnz])
    ro = np.asarray(s.RowOffsets)
    b = np.asarray(s.b, dtype=np.float64)
    f = np.float64

    def sums(terms):
        return f(0.0 + (total(terms) if len(terms) else 0.0))

    def finite(v):
        return bool(abs(v) <= DBL_BIG)

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
        rho = rr0 = sums(r * r)
        res = float(np.sqrt(rr0))
        shown = float(np.sqrt(rr0 / rr0)) if rule == _lib.RULE_VIENNACL else res
        trace = [shown]
        if not (0.0 < rr0 <= DBL_BIG):
            return closing(x, 0, res, _lib.NONFINITE, trace)
        k = 0
        while True:
            phat = minv(p)                                                    # the cycle p -> phat
            v = row_sums(e, c, ro, phat)
            sigma = sums(rhat * v)
            alpha = rho / sigma
            if sigma == 0.0 or not finite(sigma) or not finite(alpha):      # breakdown, before this body's updates: the last judged figure again
                trace.append(shown)
                return closing(x, k + 1, res, _lib.NONFINITE, trace)
            av = alpha * v
            sv = r - av                                                       # pass S
            shat = minv(sv)                                                   # the cycle s -> shat
            t = row_sums(e, c, ro, shat)
            theta = sums(sv * t)                                              # with the unhatted s
            tau = sums(t * t)
            omega = f(0.0) if tau == 0.0 else theta / tau
            if not finite(omega):
                trace.append(shown)
                return closing(x, k + 1, res, _lib.NONFINITE, trace)
            ap = alpha * phat                                                 # pass X
            x1 = x + ap
            os_ = omega * shat
            x = x1 + os_
            ot = omega * t
            r = sv - ot
            rr = sums(r * r)
            rhon = sums(rhat * r)
            res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, k + 1, rr, rr0)      # pass P
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
            rho = rhon
            k += 1


# --------------------------------------------------------------------------- the systems and hierarchies of the two test files
# name -> (the name in tests/test_bicgstab_host.py, or a builder), symmetric?
TABLE = {
    "convdiff16": ("convdiff16", False),                                             # 16^3, c = (.5, .25, 0)
    "convdiff16strong": ("convdiff16strong", False),                                 # 16^3, c = (.9, .9, .9)
    "upwind16": ("upwind16", False),                                                 # 16^3 upwind, c = (2, 1, .5)
    "convdiff32x32": ("convdiff32x32", False),                                       # 32^2, c = (.5, .25)
    "convdiff12x10x8": (lambda: problems.convection_diffusion(12, 10, 8, (0.5, 0.25, 0.1)), False),
    "poisson16": ("poisson16", True),
}
NONSYMMETRIC = [name for name, (_, symmetric) in TABLE.items() if not symmetric]
RHS = ("ones", "randn")
MAPS = ("box", "agg")
SOURCES = ("own", "sym")
_cache = {}


def system(name, rhs="randn"):
    """The table's system with b = A.1 ("ones") or an N(0,1) b of fixed seed ("randn"); x0 = 0; the grid is kept."""
    key = ("system", name, rhs)
    if key not in _cache:
        source = TABLE[name][0]
        if isinstance(source, str):
            _cache[key] = bicgstab_system(source, rhs)[0]
        else:
            s = source()
            b = _product(s, np.ones(s.Count)) if rhs == "ones" else np.random.default_rng(SEED).standard_normal(s.Count)
            _cache[key] = with_b(s, b, f"{name}-{rhs}")
    return _cache[key]


def class_omega(grid):
    """ConjugateGradientMgGpu's default omega."""
    return 6.0 / 7.0 if grid[2] > 1 else 4.0 / 5.0


def source_matrix(name, source):
    """The system whose matrix the hierarchy is built from: the system's own, or its symmetric part."""
    key = ("source", name, source)
    if key not in _cache:
        s = system(name)
        _cache[key] = s if source == "own" else problems.symmetric_part(s)
    return _cache[key]


def hierarchy(name, maps, source):
    """The yardstick hierarchy, built once per (system, maps, source): 'box' is the geometric set-up's (3 levels, the class's omega),
    'agg' the aggregation class's defaults."""
    key = ("H", name, maps, source)
    if key not in _cache:
        m = source_matrix(name, source)
        if maps == "box":
            _cache[key] = Hierarchy(*csr_of(m), maps=box_maps(m.grid, 3), omega=class_omega(m.grid))
        else:
            _cache[key] = Hierarchy(*csr_of(m))
    return _cache[key]


def level(s, rel=1e-8):
    return rel * float(np.linalg.norm(s.b))


def run(name, rhs, maps, source, rule=_lib.RULE_CSHARP, rel=1e-8, **kw):
    """The yardstick's run to a relative ``rel``, computed once and shared (nothing changes it)."""
    key = ("run", name, rhs, maps, source, rule, rel, tuple(sorted(kw.items())))
    if key not in _cache:
        s = system(name, rhs)
        tol = rel if rule == _lib.RULE_VIENNACL else level(s, rel)
        _cache[key] = pbicgstab_oracle(s, hierarchy(name, maps, source).apply, rule, tol, **{"max_it": MAX_IT, **kw})
    return _cache[key]


def plain(name, rhs):
    key = ("plain", name, rhs)
    if key not in _cache:
        s = system(name, rhs)
        _cache[key] = bicgstab_oracle(s, None, _lib.RULE_CSHARP, level(s), max_it=MAX_IT)
    return _cache[key]


def equal_runs(a, b):
    same = lambda u, v: u == v or (math.isnan(u) and math.isnan(v))
    return (a["status"] == b["status"] and a["iteration"] == b["iteration"] and same(a["residual"], b["residual"]) and
            same(a["true_residual"], b["true_residual"]) and np.array_equal(a["trace"], b["trace"], equal_nan=True) and
            np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["r"], b["r"], equal_nan=True))


# --------------------------------------------------------------------------- 1. the restatement is bicgstab_oracle's
@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_a_diagonal_or_the_identity_as_callable_equals_bicgstab_oracle_bit_for_bit(rule):
    s, _ = bicgstab_system("random_nonsymmetric5000", "randn")
    dinv = 1.0 / diagonal_of(s)
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else level(s)
    jacobi = bicgstab_oracle(s, dinv, rule, tol, max_it=MAX_IT)
    assert jacobi["status"] == _lib.OK and jacobi["iteration"] >= 3
    assert equal_runs(pbicgstab_oracle(s, lambda v: dinv * v, rule, tol, max_it=MAX_IT), jacobi)
    identity = bicgstab_oracle(s, None, rule, tol, max_it=MAX_IT)
    assert identity["status"] == _lib.OK and identity["iteration"] != jacobi["iteration"]
    assert equal_runs(pbicgstab_oracle(s, lambda v: v, rule, tol, max_it=MAX_IT), identity)


def test_other_sums_and_a_start_vector_equal_bicgstab_oracle_too():
    s = system("convdiff32x32", "randn")
    dinv = 1.0 / diagonal_of(s)
    x0 = 0.5 * np.cos(0.01 * np.arange(s.Count))
    pairwise = lambda terms: float(np.sum(terms)) if len(terms) else 0.0
    for kw in (dict(total=pairwise), dict(x0=x0), dict(min_it=40), dict(tol=0.0, max_it=3)):
        kw = {"tol": level(s), "max_it": MAX_IT, **kw}
        assert equal_runs(pbicgstab_oracle(s, lambda v: dinv * v, **kw), bicgstab_oracle(s, dinv, **kw)), kw


# --------------------------------------------------------------------------- 2. the table's systems
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name", list(TABLE))
def test_the_true_residual_is_within_the_stop_level(name, rhs, maps, source):
    """The condition on the chosen inputs that makes the factor 1.001 of the GPU tests safe, as in tests/test_bicgstab_host.py."""
    s = system(name, rhs)
    o = run(name, rhs, maps, source)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs} {maps} {source}: {o['iteration']} bodies (plain {plain(name, rhs)['iteration']}), recurrence {o['residual']:.3e}, "
          f"true {true:.3e} = {true / level(s):.4f} x the stop level, |true - recurrence| = {abs(true - o['residual']) / level(s):.2e} x the level")
    assert o["status"] == _lib.OK
    assert o["residual"] < level(s)
    assert true <= 1.001 * level(s)
    assert abs(true - o["residual"]) <= 1e-4 * level(s)
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name", NONSYMMETRIC)
def test_the_hierarchy_of_the_matrix_itself_needs_fewer_bodies_than_the_plain_loop(name, rhs, maps):
    """Counts are not pinned: they move with the summation order."""
    own, bare = run(name, rhs, maps, "own"), plain(name, rhs)
    print(f"{name} {rhs} {maps}: own {own['iteration']} bodies, symmetric part {run(name, rhs, maps, 'sym')['iteration']}, plain {bare['iteration']}")
    assert bare["status"] == _lib.OK and own["iteration"] < bare["iteration"]


def test_on_a_symmetric_matrix_both_hierarchies_are_one():
    for maps in MAPS:
        assert equal_runs(run("poisson16", "randn", maps, "own"), run("poisson16", "randn", maps, "sym"))


# --------------------------------------------------------------------------- 3. rules, cap, minimum, corner cases
@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_four_rules_stop_the_yardstick(rule):
    s = system("convdiff16", "randn")
    minv = hierarchy("convdiff16", "box", "own").apply
    start = with_b(s, s.b, "nonzero-start")
    start.x[:] = 0.5
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else level(s)
    o = pbicgstab_oracle(start, minv, rule, tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] >= 3
    zero = run("convdiff16", "randn", "box", "own", rule)
    # MGCG_RULE_SIMPLE starts from x = 0 whatever the caller's x holds
    assert equal_runs(o, zero) == (rule == _lib.RULE_SIMPLE)
    if rule == _lib.RULE_VIENNACL:
        assert o["trace"][-1] < tol <= o["trace"][-2] and zero["trace"][0] == 1.0
    else:
        assert o["residual"] < tol and o["trace"][-1] == o["residual"]


def test_the_iteration_cap_and_the_minimum_are_kept():
    s = system("convdiff16", "randn")
    minv = hierarchy("convdiff16", "box", "own").apply
    capped = pbicgstab_oracle(s, minv, tol=0.0, max_it=3)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == 4 and len(capped["trace"]) == 5
    tol = 1e-2 * float(np.linalg.norm(s.b))
    free = pbicgstab_oracle(s, minv, tol=tol, max_it=400)
    held = pbicgstab_oracle(s, minv, tol=tol, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5


def test_the_corner_cases_of_the_method_with_the_identity_as_a_callable():
    identity = lambda v: v
    s = system("convdiff16", "randn")
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        zero = pbicgstab_oracle(with_b(s, np.zeros(s.Count), "b0"), identity, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)
    s = sigma_zero2()
    o = pbicgstab_oracle(s, identity, tol=1e-12)
    root2 = math.sqrt(2.0)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], s.x)
    assert list(o["trace"]) == [root2, root2] and o["residual"] == root2 and o["true_residual"] == root2
    s = rho_zero2()
    o = pbicgstab_oracle(s, identity, tol=0.0)
    assert o["status"] == _lib.NONFINITE and o["iteration"] == 1
    assert np.array_equal(o["x"], [0.5, 0.0]) and o["residual"] == 0.0 and o["true_residual"] == 0.0 and list(o["trace"]) == [root2, 0.0]
    ok = pbicgstab_oracle(s, identity, tol=1e-12)
    assert ok["status"] == _lib.OK and ok["iteration"] == 1 and np.array_equal(ok["x"], [0.5, 0.0])


# --------------------------------------------------------------------------- 4. the symmetric part
def test_symmetric_part_gives_poisson_on_the_central_stencil():
    for dims, c in (((16, 16, 16), (0.5, 0.25, 0.0)), ((16, 16, 16), (0.9, 0.9, 0.9)), ((32, 32, 1), (0.5, 0.25)), ((12, 10, 8), (0.5, 0.25, 0.1)), ((5, 4, 3), (0.3, 0.7, 0.1))):
        s = problems.convection_diffusion(*dims, c)
        half, p = problems.symmetric_part(s), problems.poisson(*dims)
        assert np.array_equal(half.Elements, p.Elements) and np.array_equal(half.ColumnIndeces, p.ColumnIndeces) and np.array_equal(half.RowOffsets, p.RowOffsets), (dims, c)
        assert half.ColumnIndeces.dtype == np.int32 and half.RowOffsets.dtype == np.int32 and half.Elements.dtype == np.float64
        assert np.array_equal(half.b, s.b) and np.array_equal(half.x, s.x) and half.grid == s.grid and half.b is not s.b
    p = problems.poisson(6, 5, 4)
    again = problems.symmetric_part(p)
    assert np.array_equal(again.Elements, p.Elements) and np.array_equal(again.ColumnIndeces, p.ColumnIndeces)


def test_symmetric_part_of_the_upwind_stencil_is_symmetric_and_keeps_the_diagonal():
    s = problems.convection_diffusion(5, 4, 3, (2.0, 1.0, 0.5), upwind=True)
    half = problems.symmetric_part(s)
    a, h = s.to_scipy().toarray(), half.to_scipy().toarray()
    assert np.array_equal(h, h.T) and np.array_equal(h, (a + a.T) / 2) and not np.array_equal(a, a.T)
    assert np.array_equal(np.diag(h), np.diag(a)) and (np.diag(h) == 13.0).all()
    row = 20 + 5 + 1
    assert h[row, row - 1] == h[row - 1, row] == -3.0 and h[row, row - 5] == -2.0 and h[row, row - 20] == -1.5
    assert np.array_equal(half.RowOffsets, s.RowOffsets) and np.array_equal(half.ColumnIndeces, s.ColumnIndeces)     # the pattern was symmetric
    for i in range(half.Count):
        cols = half.ColumnIndeces[half.RowOffsets[i]: half.RowOffsets[i + 1]]
        assert (np.diff(cols) > 0).all()
    # a pattern that is not symmetric: the union, a one-way entry halved on both sides
    one = problems.LinearSystem(np.array([2.0, 1.0, 3.0]), np.array([0, 1, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32), np.zeros(2), np.ones(2), "one-way")
    assert np.array_equal(problems.symmetric_part(one).to_scipy().toarray(), [[2.0, 0.5], [0.5, 3.0]])


# --------------------------------------------------------------------------- 5. the library's host side
def test_the_symbol_is_exported_and_bound(hiplib):
    assert hasattr(hiplib, "SolveBicgstabMg") and "SolveBicgstabMg" in _lib.SIGNATURES


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import amg, bicgstab, multigrid

    assert callable(multigrid.ConjugateGradientMgGpu.SolveBicgstab) and callable(multigrid.ConjugateGradientMgGpu.ReadResidual)
    assert amg.ConjugateGradientAmgGpu.SolveBicgstab is multigrid.ConjugateGradientMgGpu.SolveBicgstab
    assert "hierarchy" in multigrid.ConjugateGradientMgGpu.SolveBicgstab.__doc__ and "TrueResidual" in multigrid.ConjugateGradientMgGpu.SolveBicgstab.__doc__
    assert "SolveBicgstabMg" in bicgstab.__doc__ and "SolveBicgstabMg" in conjugategradient_amd.__doc__
    assert callable(problems.symmetric_part)


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    """A zeroed hierarchy handle is one of 0 ranks: refused as a hierarchy of several ranks is.  The row-count refusal needs a hierarchy, and
    there is none without a device: tests/test_gpu_bicgstab_mg.py has it."""
    L = hiplib
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    handle = C.create_string_buffer(4096)                  # stands for the handles: a refused call looks at none of them
    h = C.addressof(handle)
    big, small_ = _VectorHead(None, 10, -1, b""), _VectorHead(None, 9, -1, b"")
    vec, short = C.addressof(big), C.addressof(small_)

    def call(blas=h, sparse=h, mg=h, v=vec, s=vec, t=vec, rhat=vec, rule=_lib.RULE_CSHARP):
        L.MgcgClearLastError()
        st = L.SolveBicgstabMg(blas, sparse, None, mg, vec, vec, vec, vec, vec, vec, vec, vec, v, s, t, rhat, 28, 10, 1e-8, 0, 10, rule,
                               C.byref(it), C.byref(res), C.byref(true), None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(mg=None), dict(v=None), dict(s=None), dict(t=None), dict(rhat=None)):
        st, msg = call(**kw)
        assert st == _lib.ERROR and "SolveBicgstabMg: null handle" in msg, (kw, msg)
    st, msg = call(rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "SolveBicgstabMg:" in msg
    for rule in (-1, 5):
        st, msg = call(rule=rule)
        assert st == _lib.ERROR and f"unknown stop rule {rule}" in msg
    for name in ("v", "s", "t", "rhat"):
        st, msg = call(**{name: short})
        assert st == _lib.ERROR and f"SolveBicgstabMg: the {name} vector holds 9 entries" in msg, (name, msg)
    st, msg = call()
    assert st == _lib.ERROR and "SolveBicgstabMg: the hierarchy was built for 0 rank(s); the V-cycle form runs on one rank" in msg, msg
