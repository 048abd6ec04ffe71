"""The K-cycle of the aggregation multigrid on the GPU (MgSetCycle(mg, 1, inner), ConjugateGradientAmgGpu(cycle="K", inner=...)) against its
numpy statement in tests/test_kcycle_host.py: under dot_order = 1 the cycle, SolveMg and SolveGmresMg are fixed sequences of IEEE operations
and must EQUAL the yardstick bit for bit; in the default mode the sums of the K step are tree sums and the solve is compared by iteration
count and trace.  Mode changes, the smallest and the longest coarse levels, breakdowns, refusals and the compression modes follow."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.ilu import ConjugateGradientIluGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException
from tests.gpu_util import assert_trace_close, cap_inside_a_chunk, same_bits, tuning
from tests.test_amg_host import Hierarchy, csr_of, path_graph, rows_per_level, serial_dot
from tests.test_amg_sym_host import HierarchySym, upwind
from tests.test_gmres_mg_host import fgmres_oracle
from tests.test_gpu_amg import LANES, SYSTEMS, _amg, _assert_same_solve, _classes, _irregular, _long_path, _solve, _system
from tests.test_gs_host import GsHierarchy
from tests.test_kcycle_host import INNERS, KGsHierarchy, KHierarchy, KHierarchySym

pytestmark = pytest.mark.gpu

INNER_NAMES = {0: "conjugate", 1: "minimal"}
assert {v: k for k, v in INNERS.items()} == INNER_NAMES
assert "poisson12-permuted" in SYSTEMS and "graph10" in SYSTEMS
# (system, passes) of the apply tests; "irregular" is the caller's maps of tests/test_gpu_amg.py
CASES = [("poisson12-permuted", 1), ("poisson12-permuted", 3), ("graph10", 3), ("irregular", 0)]


@functools.lru_cache(maxsize=None)
def _base(name, passes, smoother):
    """(system, constructor keywords, V yardstick) -- built once; the K forms share its levels (KCycle.of)."""
    cls = GsHierarchy if smoother == "gs" else Hierarchy
    if name == "irregular":
        s, maps, _ = _irregular()
        return s, dict(aggregates=maps), cls(*csr_of(s), maps=maps)
    s = _system(name)
    return s, dict(passes=passes), cls(*csr_of(s), passes=passes)


def _k_of(H, inner, nu=1, cycle="K", dot=serial_dot):
    K = (KGsHierarchy if isinstance(H, GsHierarchy) else KHierarchy).of(H, cycle=cycle, inner=inner, dot=dot)
    K.nu = nu
    return K


def _apply1(cg, r):
    with tuning(dot_order=1):
        return cg.Apply(r)


def _r(s, seed=5):
    return np.random.default_rng(seed).standard_normal(s.Count)


# --------------------------------------------------------------------------- 1. M^-1 r, bit for bit
@pytest.mark.parametrize("smoother", ["jacobi", "gs"])
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("inner", [0, 1])
@pytest.mark.parametrize("name,passes", CASES)
def test_apply_equals_the_yardstick_bit_for_bit(name, passes, inner, nu, smoother):
    s, kw, H = _base(name, passes, smoother)
    assert len(H.levels) >= 3, "no level qualifies for a K step: the case tests nothing"
    K = _k_of(H, inner, nu)
    r = _r(s)
    zref = K.apply(r)
    cg = _amg(s, nu=nu, smoother=smoother, cycle="K", inner=INNER_NAMES[inner], **kw)
    L = _lib.lib()
    assert L.MgCycle(cg.mg) == 1 and L.MgCycleInner(cg.mg) == inner and cg.levels == len(H.levels)
    z1 = _apply1(cg, r)
    z0 = cg.Apply(r)
    cg.Dispose()
    distance = float(np.abs(z0 - zref).max() / np.abs(zref).max())
    print(f"{name} passes {passes} inner {inner} nu {nu} {smoother}: rows {rows_per_level(H)}, branch {K.last_step['branch']}, default mode distance {distance:.2e}")
    assert K.last_step["branch"] == "both"
    assert same_bits(z1, zref)                     # (the default mode's sums are tree sums: its distance is printed, the solves below judge it)


# --------------------------------------------------------------------------- 2. SolveMg, bit for bit
@functools.lru_cache(maxsize=None)
def _reference_solve(name, inner, variant):
    s, _, H = _base(name, 3, "jacobi")
    K = _k_of(H, inner)
    b = np.asarray(s.b)
    free = K.pcg(b, dot=serial_dot)
    if variant == "plain":
        return dict(), free
    if variant == "guess":
        x0 = np.random.default_rng(8).standard_normal(s.Count)
        return dict(x0=x0), K.pcg(b, x0=x0, dot=serial_dot)
    if variant == "min-iteration":
        min_it = free["iteration"] + 4
        return dict(min_it=min_it), K.pcg(b, dot=serial_dot, min_it=min_it)
    cap = cap_inside_a_chunk(0, free["iteration"])
    return dict(max_it=cap), K.pcg(b, dot=serial_dot, max_it=cap)


@pytest.mark.parametrize("variant", ["plain", "guess", "min-iteration", "cap"])
@pytest.mark.parametrize("name,inner", [("poisson12-permuted", 0), ("poisson12-permuted", 1), ("graph10", 0)])
def test_solve_equals_the_yardstick_loop_bit_for_bit(name, inner, variant):
    """dot_order = 1: trace, iteration, residual, status and x of SolveMg on a K handle equal KHierarchy.pcg with serial dots: the loop
    keeps its standard beta."""
    s, kw, _ = _base(name, 3, "jacobi")
    how, ref = _reference_solve(name, inner, variant)
    print(f"{name} inner {inner} {variant}: yardstick iteration {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == (_lib.MAXIT_EXCEEDED if variant == "cap" else _lib.OK)
    with tuning(dot_order=1):
        cg = _amg(s, cycle="K", inner=INNER_NAMES[inner], **how, **kw)
        got = _solve(cg)
        cg.Dispose()
    _assert_same_solve(got, ref, (name, inner, variant))


def test_default_sums_give_the_yardsticks_iteration_count_and_trace():
    s, kw, H = _base("poisson12-permuted", 3, "jacobi")
    for inner in (0, 1):
        ref = _k_of(H, inner, dot=None).pcg(np.asarray(s.b))
        cg = _amg(s, cycle="K", inner=INNER_NAMES[inner], **kw)
        got = _solve(cg)
        cg.Dispose()
        v = H.pcg(np.asarray(s.b))
        print(f"inner {inner}: iterations K {got['iteration']}, yardstick {ref['iteration']}, V yardstick {v['iteration']}")
        assert got["status"] == _lib.OK and got["iteration"] == ref["iteration"]
        assert_trace_close(got["trace"], ref["trace"])
        assert np.linalg.norm(s.b - s.to_scipy() @ got["x"]) < 2e-8


# --------------------------------------------------------------------------- 3. SolveGmresMg, bit for bit
def _gmres(cg, m=9, orth=2):
    try:
        cg.SolveGmres(trace=True, m=m, orth=orth)
    except ApplicationException:
        assert cg.status == _lib.MAXIT_EXCEEDED
    cg.Read()
    return dict(x=cg.x.copy(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual, status=cg.status, trace=np.asarray(cg.trace).copy())


@pytest.mark.parametrize("case", ["poisson12-permuted", "upwind10-symmetric-strength"])
def test_flexible_gmres_equals_the_yardstick_bit_for_bit(case):
    """SolveGmresMg(m = 9, orth = 2) under dot_order = 1 against fgmres_oracle with the K apply; the upwind stencil (A != A^T) with the
    hierarchy matched on the symmetric part and minimal-residual inner steps."""
    if case == "poisson12-permuted":
        s, kw, H = _base(case, 3, "jacobi")
        K, inner = _k_of(H, 0), 0
    else:
        s = upwind(10)
        s.b = np.random.default_rng(1).standard_normal(s.Count)
        kw, inner = dict(passes=2, strength="symmetric"), 1
        K = KHierarchySym.of(HierarchySym(*csr_of(s), passes=2), inner=1, dot=serial_dot)
    assert len(K.levels) >= 3
    ref = fgmres_oracle(s, 9, 2, K.apply, tol=1e-8, max_it=400)
    with tuning(dot_order=1):
        cg = _amg(s, max_it=400, cycle="K", inner=INNER_NAMES[inner], **kw)
        got = _gmres(cg)
        cg.Dispose()
    print(f"{case}: Arnoldi steps {got['iteration']}, yardstick {ref['iteration']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    assert (got["status"], got["iteration"]) == (ref["status"], ref["iteration"])
    assert got["residual"] == ref["residual"] and got["true_residual"] == ref["true_residual"]
    assert same_bits(got["trace"], ref["trace"]) and same_bits(got["x"], ref["x"])


# --------------------------------------------------------------------------- 4. the smallest and the longest coarse levels
@pytest.mark.parametrize("inner", [0, 1])
@pytest.mark.parametrize("n", [11, 1077])
def test_k_steps_on_levels_of_two_rows_and_of_lengths_no_multiple_of_64(n, inner):
    """A path, one pass a level.  11 rows with minCoarse = 1 coarsen to 7, 4, 2 and 1: K steps on levels of 7, 4 and 2 rows, one row on the
    last.  1077 rows on five levels coarsen to 617, 352, 202 and 114: more than one workgroup and no C of a multiple of 64 rows."""
    s = path_graph(n, 5)
    how = dict(passes=1, minCoarse=1, levels=16) if n == 11 else dict(passes=1, levels=5)
    H = Hierarchy(*csr_of(s), **how)
    rows = rows_per_level(H)
    print(n, rows)
    assert len(rows) >= 4 and all(r % 64 for r in rows[1:-1])
    assert (rows[-1] == 1 and any(r in (2, 3) for r in rows[1:-1])) if n == 11 else rows[1] > 256
    K = _k_of(H, inner)
    cg = _amg(s, cycle="K", inner=INNER_NAMES[inner], **how)
    assert cg.levels == len(rows)
    for seed in (5, 6):
        r = _r(s, seed)
        assert same_bits(_apply1(cg, r), K.apply(r)), seed
    with tuning(dot_order=1):
        got = _solve(cg)
    cg.Dispose()
    _assert_same_solve(got, K.pcg(np.asarray(s.b), dot=serial_dot), (n, inner))


def _reassociation_bound(K):
    """What another order of summation may move the answer of a cycle with ONE K step by, relative to max |z|.  A sum of n terms added in
    another order moves by at most n 2^-53 of the sum of the terms' magnitudes, that is by n 2^-53 kappa of itself with kappa = sum |t| /
    |sum t|.  a1, k1 and k2 are products and quotients of the five sums (first order: their relative moves add: at most 5 n 2^-53 kappa_max),
    rr = b_c - a1 v1 moves by that times |a1 v1| <= 2 |b_c| or so, the second cycle and product are linear and do not amplify, and e is
    linear in k1, k2, c2: fewer than 20 such moves reach e, and the post-smoothing sweeps contract.  100 n 2^-53 kappa_max leaves a factor 5."""
    st = K.last_step
    u1, u2 = (st["v1"], st["v2"]) if K.inner else (st["c1"], st["c2"])
    kappa = max(float(np.abs(x * y).sum() / abs((x * y).sum())) for x, y in ((u1, st["v1"]), (u1, st["b"]), (u2, st["v1"]), (u2, st["v2"]), (u2, st["rr"])))
    return 100.0 * len(st["b"]) * 2.0 ** -53 * kappa, kappa


def test_every_stride_loop_of_the_k_passes_takes_a_second_trip():
    """The path of 2 * 2048 * 256 + 1077 rows of tests/test_gpu_amg.py, three levels, one pass a level: level 1, the C of the one K step, has
    more rows than kMaxGrid * kBlock lanes, so the sums passes, the residual pass and the combine pass all come round again -- in the
    default mode too, whose sums are then the sums of 2048 partial sums (a trip left out would move z by a part of itself, not by the
    rounding that _reassociation_bound allows)."""
    s, H = _long_path("uniform")
    rows = rows_per_level(H)
    assert len(rows) == 3 and rows[1] > LANES, rows
    r = _r(s)
    cg = _amg(s, levels=3, passes=1, cycle="K")
    for inner in (0, 1):
        assert _lib.lib().MgSetCycle(cg.mg, 1, inner) == 0
        K = _k_of(H, inner)
        zref = K.apply(r)
        assert K.last_step["branch"] == "both"
        assert same_bits(_apply1(cg, r), zref), inner
        z0 = cg.Apply(r)
        distance = float(np.abs(z0 - zref).max() / np.abs(zref).max())
        bound, kappa = _reassociation_bound(K)
        print(f"inner {inner}: rows {rows}, default mode distance {distance:.2e}, bound {bound:.2e} (kappa {kappa:.1f})")
        assert distance <= bound
    cg.Dispose()


# --------------------------------------------------------------------------- 5. modes
def test_mode_round_trips_and_hierarchies_without_a_k_level():
    L = _lib.lib()
    s, kw, H = _base("poisson12-permuted", 3, "jacobi")
    r = _r(s)
    zv = H.apply(r)
    cg = _amg(s, **kw)
    assert L.MgCycle(cg.mg) == 0 and L.MgCycleInner(cg.mg) == 0 and same_bits(_apply1(cg, r), zv)
    for inner in (0, 1, 1, 0):                                                    # V -> K -> K (the same, then another inner) -> V
        assert L.MgSetCycle(cg.mg, 1, inner) == 0 and L.MgCycle(cg.mg) == 1 and L.MgCycleInner(cg.mg) == inner
        assert same_bits(_apply1(cg, r), _k_of(H, inner).apply(r)), inner
        assert same_bits(_apply1(cg, r), _k_of(H, inner).apply(r)), inner
    assert L.MgSetCycle(cg.mg, 0, 1) == 0 and L.MgCycle(cg.mg) == 0 and L.MgCycleInner(cg.mg) == 0
    assert same_bits(_apply1(cg, r), zv)
    with tuning(dot_order=1):
        got = _solve(cg)
    _assert_same_solve(got, H.pcg(np.asarray(s.b), dot=serial_dot), "back in V mode")
    # a value outside the modes is refused and changes nothing
    L.MgcgClearLastError()
    assert L.MgSetCycle(cg.mg, 2, 0) == -1 and "MgSetCycle: cycle 2" in _lib.last_error() and L.MgCycle(cg.mg) == 0
    L.MgcgClearLastError()
    cg.Dispose()
    for levels in (2, 1):                                                         # no level qualifies: the V-cycle bit for bit
        V = Hierarchy(*csr_of(s), passes=3, levels=levels)
        assert len(V.levels) == levels
        cg = _amg(s, passes=3, levels=levels, cycle="K", inner="minimal")
        assert L.MgCycle(cg.mg) == 1 and cg.levels == levels
        assert same_bits(_apply1(cg, r), V.apply(r)) and same_bits(cg.Apply(r), _amg_apply_v(s, r, passes=3, levels=levels))
        cg.Dispose()


def _amg_apply_v(s, r, **kw):
    cg = _amg(s, **kw)
    z = cg.Apply(r)
    cg.Dispose()
    return z


# --------------------------------------------------------------------------- 6. breakdowns
@pytest.mark.parametrize("order", [0, 1])
def test_zero_gives_plus_zero_and_a_nan_comes_back(order):
    s, kw, H = _base("poisson12-permuted", 3, "jacobi")
    for smoother in ("jacobi", "gs"):
        for inner in (0, 1):
            cg = _amg(s, smoother=smoother, cycle="K", inner=INNER_NAMES[inner], **kw)
            with tuning(dot_order=order):
                z = cg.Apply(np.zeros(s.Count))
                assert same_bits(z, np.zeros(s.Count)), (smoother, inner)
                r = _r(s)
                r[s.Count // 3] = np.nan
                z = cg.Apply(r)                                                    # returns: every launch is enqueued whatever the data
                assert z.shape == (s.Count,) and not np.isfinite(z).all()
                if smoother == "jacobi" and order == 1:
                    assert same_bits(cg.Apply(_r(s)), _k_of(H, inner).apply(_r(s)))          # ... and the handle is as good as before
            cg.Dispose()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals_carry_a_message_and_leave_the_handle_usable():
    L = _lib.lib()
    g = problems.poisson(8, 8, 4)
    geo = ConjugateGradientMgGpu(g.Count, 7, 0, 500, 1e-8, g.grid).load(g)
    geo.Initialize()
    r = _r(g)
    before = geo.Apply(r)
    for cycle in (0, 1):
        L.MgcgClearLastError()
        assert L.MgSetCycle(geo.mg, cycle, 0) == -1 and "MgSetCycle" in _lib.last_error() and "built from a grid" in _lib.last_error()
    L.MgcgClearLastError()
    assert L.MgCycle(geo.mg) == 0 and same_bits(geo.Apply(r), before)
    geo.Dispose()
    ilu = ConjugateGradientIluGpu(g.Count, 7, 0, 500, 1e-8).load(g)
    ilu.Initialize()
    before = ilu.Apply(r)
    assert L.MgSetCycle(ilu.mg, 1, 0) == -1 and "MgSetCycle" in _lib.last_error() and "ILU(0)" in _lib.last_error()
    L.MgcgClearLastError()
    assert L.MgCycle(ilu.mg) == 0 and same_bits(ilu.Apply(r), before)
    ilu.Dispose()
    # the loops that need a fixed linear map refuse a K handle at entry; the handle and x stay as they were
    s, kw, H = _base("poisson12-permuted", 3, "jacobi")
    K = _k_of(H, 0)
    r = _r(s)
    cg = _amg(s, cycle="K", **kw)
    cg.Read()
    x0 = cg.x.copy()
    for call in (lambda: cg.SolveMinres(), lambda: cg.SolveBicgstab(), lambda: cg.SolveLobpcg(2)):
        with pytest.raises(_lib.MgcgError, match="MgSetCycle"):
            call()
        L.MgcgClearLastError()
        cg.Read()
        assert same_bits(cg.x, x0) and L.MgCycle(cg.mg) == 1
        assert same_bits(_apply1(cg, r), K.apply(r))
    # ... and take it again in V mode
    assert L.MgSetCycle(cg.mg, 0, 0) == 0
    cg.SolveBicgstab()
    assert cg.status == _lib.OK
    cg.Dispose()


# --------------------------------------------------------------------------- 8. compression modes
@functools.lru_cache(maxsize=None)
def _plain_form(name):
    s, kw, _ = _base(name, 3, "jacobi")
    cg = _amg(s, compression=0, cycle="K", **kw)
    out = _everything(cg, s)
    cg.Dispose()
    return out


def _everything(cg, s):
    out = dict(classes=_classes(cg))
    with tuning(dot_order=1):
        out["apply"] = cg.Apply(_r(s))
        out["solve"] = _solve(cg)
    return out


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10"])
def test_matrix_compression_changes_no_bit(name, mode):
    """The lossless forms of MgcgSetMatrixCompression serve the K step's products v = A_C c as they serve the cycle's passes: under
    dot_order = 1 M^-1 r and the solve are the same bits in every mode, and equal the yardstick."""
    s, kw, H = _base(name, 3, "jacobi")
    plain = _plain_form(name)
    cg = _amg(s, compression=mode, cycle="K", **kw)
    got = _everything(cg, s)
    cg.Dispose()
    print(f"{name} mode {mode}: analysis classes {got['classes']}, mode 0 {plain['classes']}")
    assert not any(plain["classes"])
    if name == "graph10":
        assert max(got["classes"]) >= 1, "no level took a compressed form: the case tests nothing"
    assert same_bits(got["apply"], plain["apply"]) and same_bits(got["apply"], _k_of(H, 0).apply(_r(s)))
    for key in ("status", "iteration", "residual"):
        assert got["solve"][key] == plain["solve"][key], key
    assert same_bits(got["solve"]["trace"], plain["solve"]["trace"]) and same_bits(got["solve"]["x"], plain["solve"]["x"])
    _assert_same_solve(got["solve"], _reference_solve(name, 0, "plain")[1], (name, mode))
