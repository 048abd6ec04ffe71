"""The K-cycle of the aggregation multigrid (MgSetCycle(mg, 1, inner)) on the host side, no GPU needed: the numpy yardstick of
tests/test_gpu_kcycle.py lives here.

``KCycle`` states the K step of include/MgcgGpu.h (MgSetCycle) in np.float64 on top of any yardstick hierarchy: wherever a cycle asks the
next level C for its coarse correction and C has a map of its own, two Krylov steps preconditioned by C's cycle answer -- every named
quantity of the header one rounded operation, every sum through ``dot`` (numpy's by default; ``serial_dot`` is the library under
dot_order = 1), the breakdown rules as the header words them.  ``KHierarchy`` is ``Hierarchy`` (tests/test_amg_host.py) with it,
``KGsHierarchy`` the Gauss-Seidel hierarchy (tests/test_gs_host.py), ``KHierarchySym`` the one matched on the symmetric part
(tests/test_amg_sym_host.py).  With ``cycle="V"`` each is its parent.  The HIP cycle must EQUAL them under dot_order = 1."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import Hierarchy, csr_of, graph_laplacian, permuted, rows_per_level, serial_dot
from tests.test_amg_sym_host import HierarchySym, upwind
from tests.test_gmres_mg_host import fgmres_oracle
from tests.test_gs_host import GsHierarchy
from tests.test_mixed_host import row_sums

DBL_BIG = 1.79e308                       # the library's "finite": |v| <= 1.79e308 (csrc/vec_passes.hpp)
INNERS = {"conjugate": 0, "minimal": 1}


def _positive_finite(v):
    return bool(0.0 < v <= DBL_BIG)


# --------------------------------------------------------------------------- the yardstick
class KCycle:
    """Mixin in front of a yardstick hierarchy: ``cycle`` "V" or "K", ``inner`` 0 (conjugate) or 1 (minimal residual), ``dot(u, v)`` forms
    every sum of the K step.  ``last_step`` keeps the scalars and vectors of the outermost K step of the last apply (for the tests here)."""

    def __init__(self, *args, cycle="K", inner=0, dot=None, **kw):
        super().__init__(*args, **kw)
        assert cycle in ("V", "K") and inner in (0, 1)
        self.cycle, self.inner = cycle, inner
        self.dot = (lambda u, v: float(u @ v)) if dot is None else dot
        self.last_step = None

    @classmethod
    def of(cls, H, cycle="K", inner=0, dot=None):
        """The K form of a hierarchy that exists (an instance of this class's parent): its levels are shared, not built again."""
        K = cls.__new__(cls)
        K.__dict__.update(H.__dict__)
        K.cycle, K.inner, K.last_step = cycle, inner, None
        K.dot = (lambda u, v: float(u @ v)) if dot is None else dot
        return K

    def _vcycle(self, l, b):
        # level l > 0 is asked for a coarse correction: the K step answers when the level has a map of its own
        if self.cycle != "K" or l == 0 or l == len(self.levels) - 1:
            return super()._vcycle(l, b)
        return self.kstep(l, b)

    def kstep(self, l, b):
        """e of the K step on level C = l for the right-hand side b (the header's formulas, one rounding each)."""
        L = self.levels[l]
        f = np.float64
        cycle = super()._vcycle
        product = lambda x: row_sums(L["e"], L["c"], L["ro"], x)
        u = (lambda c, v: v) if self.inner else (lambda c, v: c)
        with np.errstate(all="ignore"):
            c1 = cycle(l, b)
            v1 = product(c1)
            u1 = u(c1, v1)
            rho1, beta1 = f(self.dot(u1, v1)), f(self.dot(u1, b))
            a1 = beta1 / rho1
            live1 = _positive_finite(rho1)
            if live1:
                p = a1 * v1
                rr = b - p
            else:
                rr = b.copy()
            c2 = cycle(l, rr)                                         # always run: the library's launch sequence is fixed
            v2 = product(c2)
            u2 = u(c2, v2)
            gamma, beta, a2 = f(self.dot(u2, v1)), f(self.dot(u2, v2)), f(self.dot(u2, rr))
            t = gamma * gamma
            q = t / rho1
            rho2 = beta - q
            live2 = live1 and _positive_finite(rho2)
            g = gamma * a2
            d = rho1 * rho2
            h = g / d
            k1 = a1 - h
            k2 = a2 / rho2
            if live2:
                p1 = k1 * c1
                p2 = k2 * c2
                e = p1 + p2
            elif live1:
                e = a1 * c1
            else:
                e = c1.copy()
        if l == 1:
            self.last_step = dict(b=b, c1=c1, v1=v1, c2=c2, v2=v2, rr=rr, rho1=rho1, beta1=beta1, a1=a1, gamma=gamma, beta=beta, a2=a2, rho2=rho2,
                                  k1=k1, k2=k2, e=e, branch="both" if live2 else "a1 c1" if live1 else "c1")
        return e


class KHierarchy(KCycle, Hierarchy):
    pass


class KGsHierarchy(KCycle, GsHierarchy):
    pass


class KHierarchySym(KCycle, HierarchySym):
    pass


def poisson_permuted(n, seed=7, rhs_seed=1):
    s = permuted(problems.poisson(n, n, n), seed)
    s.b = np.random.default_rng(rhs_seed).standard_normal(s.Count)
    return s


# --------------------------------------------------------------------------- V mode, two levels
@pytest.mark.parametrize("make", [lambda: permuted(problems.poisson(8, 8, 8), 7), lambda: graph_laplacian(7, 3)], ids=["poisson8-permuted", "graph7"])
def test_v_mode_is_the_parent_and_two_levels_are_the_v_cycle(make):
    s = make()
    r = np.random.default_rng(5).standard_normal(s.Count)
    for nu in (1, 2):
        H = Hierarchy(*csr_of(s), passes=2, nu=nu)
        assert len(H.levels) >= 3, rows_per_level(H)
        z = H.apply(r)
        assert np.array_equal(KHierarchy(*csr_of(s), passes=2, nu=nu, cycle="V").apply(r), z)
        K = KHierarchy(*csr_of(s), passes=2, nu=nu)
        assert not np.array_equal(K.apply(r), z) and K.last_step is not None        # three levels: the K step ran and moved the answer
        for inner in (0, 1):
            two = KHierarchy(*csr_of(s), passes=2, nu=nu, levels=2, inner=inner)
            assert len(two.levels) == 2
            assert np.array_equal(two.apply(r), Hierarchy(*csr_of(s), passes=2, nu=nu, levels=2).apply(r)) and two.last_step is None
            one = KHierarchy(*csr_of(s), levels=1, inner=inner)
            assert np.array_equal(one.apply(r), Hierarchy(*csr_of(s), levels=1).apply(r))


# --------------------------------------------------------------------------- the formulas
def _extended_residuals(H, step):
    """max over j of |u_j^T (b_c - A_C e)| / (||u_j|| ||b_c||), evaluated in np.longdouble, for the e of ``step`` and for the e formed from
    the same c1 and c2 in np.longdouble throughout (products, sums, scalars and e): (float64 yardstick, long double)."""
    LD = np.longdouble
    L = H.levels[1]
    n = len(L["ro"]) - 1
    rows = np.repeat(np.arange(n), np.diff(L["ro"]))

    def product(x):
        y = np.zeros(n, dtype=LD)
        np.add.at(y, rows, L["e"].astype(LD) * x[L["c"]])
        return y

    def worst(e, u1, u2):
        res = b - product(e)
        return max(float(abs(u @ res) / (np.sqrt(u @ u) * np.sqrt(b @ b))) for u in (u1, u2))

    b, c1, c2 = (step[k].astype(LD) for k in ("b", "c1", "c2"))
    shown = worst(step["e"].astype(LD), *((step["v1"].astype(LD), step["v2"].astype(LD)) if H.inner else (c1, c2)))
    v1, v2 = product(c1), product(c2)                                 # the long-double statement: the products too
    u1, u2 = (v1, v2) if H.inner else (c1, c2)
    rho1, beta1 = u1 @ v1, u1 @ b
    a1 = beta1 / rho1
    rr = b - a1 * v1
    gamma, beta, a2 = u2 @ v1, u2 @ v2, u2 @ rr
    rho2 = beta - gamma * gamma / rho1
    k1, k2 = a1 - gamma * a2 / (rho1 * rho2), a2 / rho2
    return shown, worst(k1 * c1 + k2 * c2, u1, u2)


# Measured here (x86-64, 80-bit long double): poisson12-permuted passes 2 -- inner 0: float64 yardstick 1.71e-16; inner 1: 1.82e-16 (long
# double 1.73e-19).  graph10 passes 2 -- inner 0: 4.47e-17 (1.45e-19); inner 1: 8.46e-17 (1.32e-19).
YARDSTICK_SHOWS = 1.82e-16


@pytest.mark.parametrize("inner", [0, 1])
@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10"])
def test_the_two_steps_leave_a_residual_orthogonal_to_both_directions(name, inner):
    """inner = 0: c1^T (b_c - A_C e) = c2^T (b_c - A_C e) = 0; inner = 1: the same with v1 and v2 -- what defines k1 and k2.  Both are
    evaluated in np.longdouble, relative to ||u|| ||b_c||, for the float64 yardstick's e and for an e formed in long double from the same
    vectors.  The largest value the float64 yardstick showed over the four cases when this was written is 1.82e-16 (the list above the test);
    16 x that is allowed.  The long-double e must do 100 x better than the bound: the formulas are exact, the yardstick's distance is
    rounding.  A wrong scalar -- k1 without its correction term -- misses by more than 1e-4."""
    s = permuted(problems.poisson(12, 12, 12), 7) if name == "poisson12-permuted" else graph_laplacian(10, 3)
    H = KHierarchy(*csr_of(s), passes=2, inner=inner)
    assert len(H.levels) >= 3
    H.apply(np.random.default_rng(5).standard_normal(s.Count))
    step = H.last_step
    assert step["branch"] == "both"
    shown, extended = _extended_residuals(H, step)
    print(f"{name} inner {inner}: float64 yardstick {shown:.2e}, long double {extended:.2e}")
    assert shown <= 16 * YARDSTICK_SHOWS
    assert extended <= 16 * YARDSTICK_SHOWS / 100
    wrong = dict(step, e=step["a1"] * step["c1"] + step["k2"] * step["c2"])
    assert _extended_residuals(H, wrong)[0] > 1e-4


# --------------------------------------------------------------------------- breakdown
@pytest.mark.parametrize("inner", [0, 1])
def test_a_zero_right_hand_side_gives_plus_zero(inner):
    s = permuted(problems.poisson(8, 8, 8), 7)
    for cls in (KHierarchy, KGsHierarchy):
        H = cls(*csr_of(s), passes=2, inner=inner, dot=serial_dot)
        assert len(H.levels) >= 3
        z = H.apply(np.zeros(s.Count))
        assert np.array_equal(z, np.zeros(s.Count)) and not np.signbit(z).any()
        assert H.last_step["branch"] == "c1" and H.last_step["rho1"] == 0.0


def symmetric_path4():
    """The path of 4 rows with edge weights 2, 1, 2 and the diagonal 1.25 x the off-diagonal row sum: one pass pairs {0, 1} and {2, 3}, the
    2-row level has equal diagonals, and one more pass leaves a single row."""
    w = np.array([2.0, 1.0, 2.0])
    left, right = np.r_[0.0, w], np.r_[w, 0.0]
    e = np.stack([-left, 1.25 * (left + right), -right], axis=1).ravel()
    i = np.arange(4)
    c = np.stack([i - 1, i, i + 1], axis=1).ravel()
    keep = (c >= 0) & (c < 4)
    ro = np.r_[0, np.cumsum(keep.reshape(4, 3).sum(axis=1))]
    return problems.LinearSystem(e[keep], c[keep].astype(np.int32), ro.astype(np.int32), np.zeros(4), np.ones(4), "symmetric-path-4")


@pytest.mark.parametrize("inner", [0, 1])
def test_a_second_direction_parallel_to_the_first_takes_the_a1_c1_branch(inner):
    """Three levels of 4, 2 and 1 rows: the Krylov space of the 2-row level is two-dimensional at the most, and for b_c = (1, 1) -- by the
    symmetry of the path an eigenvector of everything the cycle does, both entries computed by the same operations on the same numbers -- it
    is one-dimensional: rr = b_c - a1 v1 is zero up to one rounding, c2 is that multiple of c1, and rho2 = beta - gamma^2 / rho1 is zero
    or a rounding of either sign, never a meaningful pivot.  Where it is <= 0 the step answers a1 c1."""
    s = symmetric_path4()
    H = KHierarchy(*csr_of(s), passes=1, minCoarse=1, inner=inner, dot=serial_dot)
    assert rows_per_level(H) == [4, 2, 1]
    e = H.kstep(1, np.ones(2))
    step = H.last_step
    print(f"inner {inner}: rr {step['rr']}, rho1 {step['rho1']!r}, rho2 {step['rho2']!r}, branch {step['branch']}")
    assert step["rho1"] > 0 and np.abs(step["rr"]).max() <= 2.0 ** -52
    if not step["rho2"] <= 0:
        pytest.fail(f"rho2 = {step['rho2']!r} > 0 here: the case no longer reaches the branch it is for")
    assert step["branch"] == "a1 c1" and np.array_equal(e, step["a1"] * step["c1"])
    x = np.linalg.solve(_dense(H.levels[1]), np.ones(2))
    assert np.abs(e - x).max() <= 1e-14 * np.abs(x).max()          # ... which is the solution: one step was exact


def _dense(L):
    n = len(L["ro"]) - 1
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(L["ro"])), L["c"]), L["e"])
    return A


# --------------------------------------------------------------------------- what it buys
def _counts(n):
    s = poisson_permuted(n)
    b = np.asarray(s.b)
    tol = 1e-8 * float(np.linalg.norm(b))
    v = Hierarchy(*csr_of(s), passes=3).pcg(b, tol=tol)
    k = KHierarchy(*csr_of(s), passes=3).pcg(b, tol=tol)
    A = s.to_scipy()
    for out in (v, k):
        assert out["status"] == _lib.OK and np.linalg.norm(b - A @ out["x"]) < 2 * tol
    return v["iteration"], k["iteration"]


def test_the_k_cycle_needs_fewer_iterations_and_its_count_does_not_grow():
    """Permuted 16^3 and 24^3 Poisson, passes = 3, b ~ N(0, 1), relative 1e-8, the yardstick PCG loop with its standard beta.  Measured here
    (Iteration, the loop's 0-based count): 16^3 V 20, K 16; 24^3 V 23, K 17."""
    v16, k16 = _counts(16)
    v24, k24 = _counts(24)
    print(f"16^3: V {v16}, K {k16}; 24^3: V {v24}, K {k24}")
    assert k16 < v16 and k24 < v24
    assert abs(k24 - k16) <= 2


def test_flexible_gmres_converges_with_the_k_cycle_on_an_upwind_stencil():
    """Upwind convection-diffusion 10^3 (A != A^T), the hierarchy matched on the symmetric part, minimal-residual inner steps."""
    s = upwind(10)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    H = KHierarchySym(*csr_of(s), passes=2, inner=1, dot=serial_dot)
    assert len(H.levels) >= 3, rows_per_level(H)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    out = fgmres_oracle(s, 10, 2, H.apply, tol=tol)
    ref = fgmres_oracle(s, 10, 2, HierarchySym(*csr_of(s), passes=2).apply, tol=tol)
    print(f"rows per level {rows_per_level(H)}; Arnoldi steps: K {out['iteration']}, V {ref['iteration']}")
    assert H.last_step is not None and H.last_step["branch"] == "both"
    assert out["status"] == _lib.OK and out["true_residual"] < 2 * tol
    assert out["iteration"] <= ref["iteration"]


# --------------------------------------------------------------------------- the library without a device
def test_exports_and_python_surface(hiplib):
    for name in ("MgSetCycle", "MgCycle", "MgCycleInner"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    from conjugategradient_amd import amg

    assert amg.CYCLES == {"V": 0, "K": 1} and amg.INNERS == INNERS
    with pytest.raises(_lib.MgcgError, match="cycle 'W'"):
        amg.ConjugateGradientAmgGpu(10, 3, 0, 10, 1e-8, cycle="W")
    with pytest.raises(_lib.MgcgError, match="inner 'steepest'"):
        amg.ConjugateGradientAmgGpu(10, 3, 0, 10, 1e-8, cycle="K", inner="steepest")


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the hierarchy: a refused call does not look at it
    h = C.addressof(handle)

    def message(call):
        L.MgcgClearLastError()
        status = call()
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return status, msg

    for cycle, inner in ((0, 0), (1, 0), (1, 1)):
        status, msg = message(lambda: L.MgSetCycle(None, cycle, inner))
        assert status == -1 and "MgSetCycle: null handle" in msg
    for cycle in (-1, 2, 7):
        status, msg = message(lambda: L.MgSetCycle(h, cycle, 0))
        assert status == -1 and f"MgSetCycle: cycle {cycle}, must be 0" in msg, msg
    for inner in (-1, 2):
        status, msg = message(lambda: L.MgSetCycle(h, 1, inner))
        assert status == -1 and f"MgSetCycle: inner {inner}, must be 0" in msg, msg
    assert L.MgCycle(None) == 0 and L.MgCycleInner(None) == 0
