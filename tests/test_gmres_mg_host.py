"""V-cycle-preconditioned flexible GMRES(m) on the host side (no GPU needed): the yardstick of tests/test_gpu_gmres_mg.py lives here and is
checked against ``gmres_oracle``, against the true residual, against ``pbicgstab_oracle`` on the two systems that loop cannot solve, and on
the corner cases of the method; the library exports the entry point and refuses bad arguments before it asks for a device.

``fgmres_oracle`` is ``gmres_oracle`` (tests/test_gmres_host.py) restated with a callable M^-1 in Saad's flexible form and the same
rounding order: the loop of include/MgcgGpu.h (SolveGmresMg) in np.float64 with z_j = minv(v_j), w = A z_j and x = x + sum y_i z_i.  The
V-cycle is ``Hierarchy.apply`` (tests/test_amg_host.py) on the hierarchies of tests/test_bicgstab_mg_host.py.  Under dot_order = 1 the HIP
loop must EQUAL it.

Combinations: every (system, right-hand side, maps, source, m, orth) of section 2 met its conditions with serial sums, so none was dropped."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import Hierarchy, box_maps, csr_of
from tests.test_bicgstab_host import DBL_BIG, MAX_IT, SEED, _product, nonsymmetric_tridiagonal, numpy_true_residual, small
from tests.test_bicgstab_mg_host import MAPS, NONSYMMETRIC, RHS, SOURCES, TABLE, class_omega, equal_runs, hierarchy, level, pbicgstab_oracle, system
from tests.test_bicgstab_mg_host import run as bicgstab_run
from tests.test_gmres_host import GROUP, MAX_M, gmres_oracle, never_increases, singular2
from tests.test_mixed_host import row_sums, serial_sum
from tests.test_sreduce_host import diagonal_of, stop_decision, with_b
from tests.test_variant_refusals_host import EIGHT, H, OUT3, STOP, _VectorHead


# --------------------------------------------------------------------------- the yardstick
def fgmres_oracle(s, m, orth, minv, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=400, x0=None, total=serial_sum):
    """A x = s.b from s.x (x0) by flexible GMRES(m), right-preconditioned with minv(v) = M^-1 v (any map); ``orth`` Gram-Schmidt passes per
    step.  total(terms): the sum of the terms (default: serial, left to right).  Returns x, r (= b - A x, the closing product), iteration
    (Arnoldi steps), residual, true_residual, status, trace; and ``gap`` as gmres_oracle does."""
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
        Z = np.empty((m, n))
        Rm = np.zeros((m, m))
        while True:                                                               # one cycle
            beta = np.sqrt(beta2)
            V[0] = r / beta
            g = [beta]
            cs, sn = [], []
            cols, ended = 0, None
            for j in range(m):
                Z[j] = minv(V[j])                                                 # the cycle v_j -> z_j, kept
                w = row_sums(e, c, ro, Z[j])
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
            # the close: y = R^-1 g over the completed columns, x += sum y_i z_i in groups of eight columns
            y = np.zeros(cols)
            for i in range(cols - 1, -1, -1):
                acc = g[i]
                for q in range(i + 1, cols):
                    t = Rm[i, q] * y[q]
                    acc = acc - t
                y[i] = acc / Rm[i, i]
            for g0 in range(0, cols, GROUP):
                g1 = min(g0 + GROUP, cols)
                terms = y[g0:g1, None] * Z[g0:g1]
                acc = np.add.accumulate(np.vstack([np.zeros((1, n)), terms]), axis=0)[-1]
                x = x + acc
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
MS = (2, 9, 20)
ORTHS = (1, 2)
_cache = {}


def run(name, rhs, maps, source, m, orth, rule=_lib.RULE_CSHARP, rel=1e-8, **kw):
    """The yardstick's run to a relative ``rel`` with serial sums, computed once and shared (nothing changes it)."""
    key = ("run", name, rhs, maps, source, m, orth, rule, rel, tuple(sorted(kw.items())))
    if key not in _cache:
        s = system(name, rhs)
        tol = rel if rule == _lib.RULE_VIENNACL else level(s, rel)
        _cache[key] = fgmres_oracle(s, m, orth, hierarchy(name, maps, source).apply, rule, tol, **{"max_it": MAX_IT, **kw})
    return _cache[key]


# The two systems SolveBicgstabMg cannot solve: a central stencil at cell Peclet number >= 2 under a Jacobi-smoothed cycle.
# name -> (c, the matrix the box hierarchy is built from, the step cap: 1.5 x the steps of the serial-sum yardstick, ones / randn)
HARD = {
    "convdiff16c2": ((2.0, 2.0, 2.0), "own"),
    "convdiff16c5": ((5.0, 5.0, 5.0), "sym"),
}


def hard_system(name, rhs):
    key = ("hard", name, rhs)
    if key not in _cache:
        s = problems.convection_diffusion(16, 16, 16, HARD[name][0])
        b = _product(s, np.ones(s.Count)) if rhs == "ones" else np.random.default_rng(SEED).standard_normal(s.Count)
        _cache[key] = with_b(s, b, f"{name}-{rhs}")
    return _cache[key]


def hard_hierarchy(name):
    key = ("hardH", name)
    if key not in _cache:
        s = hard_system(name, "ones")
        m = s if HARD[name][1] == "own" else problems.symmetric_part(s)
        _cache[key] = Hierarchy(*csr_of(m), maps=box_maps(m.grid, 3), omega=class_omega(m.grid))
    return _cache[key]


# --------------------------------------------------------------------------- 1. the restatement is gmres_oracle's
def _convdiff16():
    return system("convdiff16", "randn")


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_VIENNACL])
def test_the_identity_as_callable_equals_gmres_oracle_bit_for_bit(rule):
    s = _convdiff16()
    tol = 1e-8 if rule == _lib.RULE_VIENNACL else level(s)
    x0 = 0.5 * np.cos(0.01 * np.arange(s.Count))
    for m, orth in ((9, 2), (4, 1)):
        plain = gmres_oracle(s, m, orth, None, rule, tol, max_it=MAX_IT, x0=x0)
        assert plain["status"] == _lib.OK and plain["iteration"] > m              # at least one restart
        assert equal_runs(fgmres_oracle(s, m, orth, lambda v: v, rule, tol, max_it=MAX_IT, x0=x0), plain)


def test_other_sums_a_minimum_and_a_cap_equal_gmres_oracle_too():
    s = _convdiff16()
    pairwise = lambda terms: float(np.sum(terms)) if len(terms) else 0.0
    for kw in (dict(total=pairwise), dict(min_it=70), dict(tol=0.0, max_it=12)):
        kw = {"tol": level(s), "max_it": MAX_IT, **kw}
        assert equal_runs(fgmres_oracle(s, 9, 2, lambda v: v, **kw), gmres_oracle(s, 9, 2, None, **kw)), kw


@pytest.mark.parametrize("orth", ORTHS)
def test_a_diagonal_as_callable_has_the_jacobi_forms_trace_when_nothing_restarts(orth):
    """Without a restart the two loops differ in the close alone: the Jacobi form adds dinv (sum y_i v_i), the flexible form
    sum y_i (dinv v_i) -- another association of the same terms.  Every step in front of it (products of dinv v_j, the sums, the rotations,
    the stop decision) is the same sequence of operations, so iteration and trace are equal bit for bit and x to rounding."""
    s = system("upwind16", "randn")                                               # a diagonal that is not a power of two: 13
    dinv = 1.0 / diagonal_of(s)
    tol = level(s, 1e-2)                                                          # a level that 32 steps reach
    jacobi = gmres_oracle(s, 32, orth, dinv, tol=tol, max_it=MAX_IT)
    assert jacobi["status"] == _lib.OK and 16 < jacobi["iteration"] <= 32           # no restart, three groups of columns
    o = fgmres_oracle(s, 32, orth, lambda v: dinv * v, tol=tol, max_it=MAX_IT)
    assert o["status"] == _lib.OK and o["iteration"] == jacobi["iteration"] and np.array_equal(o["trace"], jacobi["trace"]) and o["residual"] == jacobi["residual"]
    assert np.max(np.abs(o["x"] - jacobi["x"])) <= 1e-12 * np.max(np.abs(jacobi["x"]))


# --------------------------------------------------------------------------- 2. the table's systems
@pytest.mark.parametrize("orth", ORTHS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name", list(TABLE))
def test_the_true_residual_is_within_the_stop_level(name, rhs, maps, source, m, orth):
    """The condition on the chosen inputs that makes the factor 1.001 of the GPU tests safe."""
    s = system(name, rhs)
    o = run(name, rhs, maps, source, m, orth)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs} {maps} {source} m={m} orth={orth}: {o['iteration']} steps, estimate {o['residual']:.3e}, true {true:.3e} = {true / level(s):.4f} x "
          f"the stop level, |true - estimate| = {abs(true - o['residual']) / level(s):.2e} x the level, restart gap {o['gap'] / level(s):.2e} x the level")
    assert o["status"] == _lib.OK
    assert o["residual"] < level(s)
    assert true <= 1.001 * level(s)
    assert abs(true - o["residual"]) <= 1e-4 * level(s)
    assert len(o["trace"]) == o["iteration"] + 1 and o["trace"][-1] == o["residual"]
    assert o["true_residual"] == math.sqrt(serial_sum(o["r"] * o["r"]))
    if orth == 2:
        assert never_increases(o["trace"])
    else:
        print(f"    orth = 1 trace non-increasing: {never_increases(o['trace'])}")


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name", list(TABLE))
def test_gmres_20_needs_no_more_cycles_than_bicgstab(name, rhs, maps):
    """A step is one cycle and one product, a BiCGStab body two of each.  Counts are not pinned: they move with the summation order."""
    o, old = run(name, rhs, maps, "own", 20, 2), bicgstab_run(name, rhs, maps, "own")
    print(f"{name} {rhs} {maps}: GMRES(20) {o['iteration']} steps, BiCGStab {old['iteration']} bodies")
    assert o["status"] == old["status"] == _lib.OK
    assert o["iteration"] <= 2 * old["iteration"] + 2


# --------------------------------------------------------------------------- 3. the capability
# Steps of the serial-sum yardstick (ones, randn), m = 20, orth = 2: convdiff16c2 314 / 330, convdiff16c5 412 / 419.  The cap is 1.5 x those.
OBSERVED = {("convdiff16c2", "ones"): 314, ("convdiff16c2", "randn"): 330, ("convdiff16c5", "ones"): 412, ("convdiff16c5", "randn"): 419}
BICGSTAB_BODIES = 1000                                                            # 2000 cycles and products: about five times what GMRES(20) needs


@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name", list(HARD))
def test_flexible_gmres_converges_where_preconditioned_bicgstab_does_not(name, rhs):
    s = hard_system(name, rhs)
    minv = hard_hierarchy(name).apply
    old = pbicgstab_oracle(s, minv, _lib.RULE_CSHARP, level(s), max_it=BICGSTAB_BODIES)
    print(f"{name} {rhs}: pbicgstab_oracle status {old['status']} at body {old['iteration']}")
    assert old["status"] != _lib.OK
    cap = OBSERVED[name, rhs] * 3 // 2
    o = fgmres_oracle(s, 20, 2, minv, _lib.RULE_CSHARP, level(s), max_it=cap)
    true = numpy_true_residual(s, o["x"])
    print(f"{name} {rhs}: GMRES(20) + V-cycle {o['iteration']} steps (cap {cap}), true residual {true / level(s):.4f} x the level")
    assert o["status"] == _lib.OK and true <= 1.001 * level(s)


# --------------------------------------------------------------------------- 4. rules, cap, minimum, corner cases
@pytest.mark.parametrize("m,cap", [(9, 12), (9, 8), (9, 9), (4, 3)])
def test_the_cap_ends_the_loop_with_x_closed_once(m, cap):
    """In mid-cycle, at a cycle's last step and at j = 0 behind a restart: iteration = cap + 1, and x is what ONE close made of the
    columns the cut cycle completed -- the estimate and the true residual agree."""
    s = _convdiff16()
    o = fgmres_oracle(s, m, 2, hierarchy("convdiff16", "box", "own").apply, tol=0.0, max_it=cap)
    assert o["status"] == _lib.MAXIT_EXCEEDED and o["iteration"] == cap + 1 and len(o["trace"]) == cap + 2
    true = numpy_true_residual(s, o["x"])
    assert abs(true - o["residual"]) <= 1e-10 * true


def test_the_minimum_is_kept_five_steps_beyond_convergence():
    s = _convdiff16()
    minv = hierarchy("convdiff16", "box", "own").apply
    tol = 1e-2 * float(np.linalg.norm(s.b))
    free = fgmres_oracle(s, 4, 2, minv, tol=tol, max_it=400)
    held = fgmres_oracle(s, 4, 2, minv, tol=tol, min_it=free["iteration"] + 5, max_it=400)
    assert free["status"] == held["status"] == _lib.OK and held["iteration"] == free["iteration"] + 5
    assert np.array_equal(held["trace"][: free["iteration"] + 1], free["trace"])
    assert numpy_true_residual(s, held["x"]) <= 1.001 * tol


def test_the_corner_cases_of_the_method_with_the_identity_as_a_callable():
    identity = lambda v: v
    s = nonsymmetric_tridiagonal(50)
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):                           # b = 0
        zero = fgmres_oracle(with_b(s, np.zeros(50), "b0"), 9, 2, identity, rule, tol=1e-12)
        assert zero["status"] == _lib.NONFINITE and zero["iteration"] == 0 and zero["residual"] == 0.0 and not zero["x"].any()
        assert len(zero["trace"]) == 1 and (math.isnan(zero["trace"][0]) if rule == _lib.RULE_VIENNACL else zero["trace"][0] == 0.0)
    for orth in ORTHS:                                                            # no next direction and no column
        o = fgmres_oracle(singular2(), 9, orth, identity, tol=1e-12)
        assert o["status"] == _lib.NONFINITE and o["iteration"] == 1 and np.array_equal(o["x"], [0.0, 0.0])
        assert list(o["trace"]) == [1.0, 1.0] and o["residual"] == 1.0 and o["true_residual"] == 1.0
    s = small([[1.0, 1.0], [0.0, 1.0]], [0.0, 1.0], "exhausted2", x=[0.0, 0.0])     # the Krylov space exhausted in the second step
    o = fgmres_oracle(s, 9, 2, identity, tol=0.0, min_it=5)
    assert o["status"] == _lib.OK and o["iteration"] == 2 and o["residual"] == 0.0
    assert np.allclose(o["x"], [-1.0, 1.0], rtol=1e-15, atol=1e-15)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_tiny_systems_end_cleanly(n):
    """A one-level hierarchy (its coarsest-level sweeps alone) as the map; n = 1 takes one step with hn = 0 and x exact."""
    s = nonsymmetric_tridiagonal(n)
    minv = Hierarchy(*csr_of(s), maps=[]).apply
    for m, orth in ((32, 2), (2, 1)):
        o = fgmres_oracle(s, m, orth, minv, tol=level(s), min_it=7 if n == 1 else 0)
        true = numpy_true_residual(s, o["x"])
        print(f"n = {n} m = {m} orth = {orth}: status {o['status']} after {o['iteration']} steps, true residual {true:.3e}")
        assert o["status"] == _lib.OK and true <= 1.001 * level(s)
        if m >= n:
            assert o["iteration"] <= n
        if n == 1:
            assert o["iteration"] == 1 and o["residual"] == 0.0 and np.array_equal(o["x"], [1.0])


# --------------------------------------------------------------------------- 5. the library's host side
def test_the_symbol_is_exported_and_bound(hiplib):
    assert hasattr(hiplib, "SolveGmresMg") and "SolveGmresMg" in _lib.SIGNATURES
    plain = _lib.SIGNATURES["SolveGmres"]
    assert _lib.SIGNATURES["SolveGmresMg"] == (plain[0], plain[1][:3] + [C.c_void_p] + plain[1][3:])     # the hierarchy behind matDescr


def test_python_surface_imports_without_a_gpu():
    import inspect

    import conjugategradient_amd
    from conjugategradient_amd import amg, gmres, multigrid, ssor

    fn = multigrid.ConjugateGradientMgGpu.SolveGmres
    assert amg.ConjugateGradientAmgGpu.SolveGmres is fn and ssor.ConjugateGradientSsorGpu.SolveGmres is fn
    p = inspect.signature(fn).parameters
    assert list(p) == ["self", "trace", "hierarchy", "m", "orth"] and (p["trace"].default, p["hierarchy"].default, p["m"].default, p["orth"].default) == (False, None, 20, 2)
    assert "hierarchy" in fn.__doc__ and "TrueResidual" in fn.__doc__ and "SolveGmresMg" in fn.__doc__
    assert "SolveGmresMg" in gmres.__doc__ and "SolveGmresMg" in conjugategradient_amd.__doc__


def _call(L, blas=H, sparse=H, mg=H, work=None, m=4, orth=2, rule=_lib.RULE_CSHARP, work_size=None, count=10):
    """One call with zeroed handles and vector heads of 10 entries: a refused call looks at nothing else.  (status, message)"""
    head = _VectorHead(None, (1000 if work_size is None else work_size), -1, b"")
    work = C.addressof(head) if work is None else None
    L.MgcgClearLastError()
    st = L.SolveGmresMg(blas, sparse, None, mg, *EIGHT, work, m, orth, 28, count, *STOP, rule, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    return st, msg


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    """A zeroed hierarchy handle is one of 0 ranks: refused as a hierarchy of several ranks is.  The row-count refusal needs a hierarchy, and
    there is none without a device: tests/test_gpu_gmres_mg.py has it."""
    L = hiplib
    who = "SolveGmresMg"
    for kw in (dict(blas=None), dict(sparse=None), dict(mg=None), dict(work="null")):
        st, msg = _call(L, **kw)
        assert st == _lib.ERROR and msg == f"{who}: null handle", (kw, msg)
    for m in (0, 33, -1, 100):
        st, msg = _call(L, m=m)
        assert st == _lib.ERROR and msg == f"{who}: m = {m}, must be 1 .. 32", msg
    for orth in (0, 3, -1):
        st, msg = _call(L, orth=orth)
        assert st == _lib.ERROR and msg == f"{who}: orth = {orth}, must be 1 or 2", msg
    st, msg = _call(L, rule=_lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm" in msg and "MGCG_RULE_HANDMADECL" in msg and msg.startswith(f"{who}:")
    for rule in (-1, 5):
        st, msg = _call(L, rule=rule)
        assert st == _lib.ERROR and msg == f"{who}: unknown stop rule {rule}"
    # 10 rows: slices of 10 entries, 2 m + 1 of them
    for m in (1, 8, 9, 32):
        slices = 2 * m + 1
        need = slices * 10
        st, msg = _call(L, m=m, work_size=need - 1)
        assert st == _lib.ERROR and f"{who}: the work vector holds {need - 1} entries, m = {m} needs {need} ({slices} slices of 10: the matrix has 10 rows)" in msg, msg
        st, msg = _call(L, m=m, work_size=need)                                   # long enough: the next refusal is the hierarchy's
        assert st == _lib.ERROR and "the hierarchy was built for" in msg, msg
    st, msg = _call(L)
    assert st == _lib.ERROR and msg == f"{who}: the hierarchy was built for 0 rank(s); the V-cycle form runs on one rank", msg
    # m is looked at before orth, orth before the rule, the rule before the work vector, the work vector before the hierarchy
    assert "m = 40" in _call(L, m=40, orth=7, rule=5, work_size=1)[1]
    assert "orth = 7" in _call(L, orth=7, rule=5, work_size=1)[1]
    assert "unknown stop rule 5" in _call(L, rule=5, work_size=1)[1]
    assert "the work vector holds 1 entries" in _call(L, work_size=1)[1]
    # 9 rows: slices 10 apart, so m = 3 needs 70 entries
    nine = _VectorHead(None, 9, -1, b"")
    head = _VectorHead(None, 69, -1, b"")
    L.MgcgClearLastError()
    st = L.SolveGmresMg(H, H, None, H, *([C.addressof(nine)] * 8), C.addressof(head), 3, 2, 25, 9, *STOP, _lib.RULE_CSHARP, *OUT3, None, 0)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    assert st == _lib.ERROR and "holds 69 entries, m = 3 needs 70 (7 slices of 10: the matrix has 9 rows)" in msg, msg
