"""The symmetric part on the device (MgcgSymmetricPart) and the aggregation hierarchy that matches on it (MgSetupAggregationEx with
strength = 1) against their numpy statement in tests/test_amg_sym_host.py: S, the maps, the level matrices, D^-1 and -- under
dot_order = 1 -- the V-cycle and the two nonsymmetric solvers behind it are compared bit for bit."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, amg, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.solver import ConjugateGradientGpu, _ptr
from tests.gpu_util import dvec, ivec, tuning
from tests.test_amg_host import Hierarchy, csr_of, reversed_rows, rows_per_level, with_duplicates
from tests.test_amg_sym_host import HierarchySym, NONSYMMETRIC, central, one_way_pair, symmetric_part_arrays, upwind, with_a_diagonal_only_row
from tests.test_bicgstab_mg_host import level, pbicgstab_oracle
from tests.test_gmres_mg_host import fgmres_oracle
from tests.test_gpu_amg import _assert_apply_equals, _assert_equal_hierarchies
from tests.test_gpu_bicgstab_mg import assert_equal_runs
from tests.test_gpu_gmres_mg import finish
from tests.test_sreduce_host import with_b

pytestmark = pytest.mark.gpu


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def _maxnz(s):
    return int(np.diff(s.RowOffsets).max())


def _amg(s, tol=1e-8, max_it=400, **kw):
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, max_it, tol, **kw).load(s)
    cg.Initialize()
    return cg


def _randn(s, seed=20261020):
    return with_b(s, np.random.default_rng(seed).standard_normal(s.Count), s.name + "-randn")


# --------------------------------------------------------------------------- 1. MgcgSymmetricPart
def _one():
    return problems.LinearSystem(np.array([4.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.zeros(1), np.ones(1), "one")


PART = {
    **NONSYMMETRIC,                                                                   # 12 x 10 x 8 central and upwind, random 1500
    "random1037": lambda: problems.random_nonsymmetric(1037),                         # no multiple of 64 or 256
    "upwind-reversed": lambda: reversed_rows(NONSYMMETRIC["upwind12x10x8"]()),
    "upwind-duplicates": lambda: with_duplicates(NONSYMMETRIC["upwind12x10x8"]()),
    "mgcg_main600": lambda: problems.mgcg_main(600),                                  # 159 entries a row, the diagonal stored first
    "one": _one,
    "one-way-pair": one_way_pair,
    "diagonal-only-row": with_a_diagonal_only_row,
}


class _Device:
    """A system's CSR arrays in device vectors of the library, the two handles, and output vectors of a given capacity."""

    def __init__(self, s, capacity):
        self.n, self.nnz, self.capacity = s.Count, s.nnz, capacity
        self.blas, self.sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
        e, c, ro = csr_of(s)
        self.a, self.ro, self.ci = dvec(e), ivec(ro), ivec(c)
        self.sa, self.sro, self.sci = dvec(np.full(max(capacity, 1), 7.0)), ivec(np.full(self.n + 1, -7)), ivec(np.full(max(capacity, 1), -7))

    def call(self, count_only=False, capacity=None):
        L = _lib.lib()
        L.MgcgClearLastError()
        out = (None, None, None) if count_only else (self.sa.Ptr, self.sro.Ptr, self.sci.Ptr)
        got = L.MgcgSymmetricPart(self.blas, self.sparse, self.a.Ptr, self.ro.Ptr, self.ci.Ptr, self.nnz, self.n, *out,
                                  self.capacity if capacity is None else capacity)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return got, msg

    def arrays(self, count):
        return self.sa.to_numpy(max(self.capacity, 1))[:count], self.sci.to_numpy(max(self.capacity, 1))[:count], self.sro.to_numpy(self.n + 1)

    def dispose(self):
        for v in (self.a, self.ro, self.ci, self.sa, self.sro, self.sci):
            v.Dispose()
        _lib.lib().DestroyBlas(self.blas)
        _lib.lib().DestroySparse(self.sparse)


@pytest.mark.parametrize("name", list(PART))
def test_symmetric_part_equals_the_yardstick_bit_for_bit(name):
    s = PART[name]()
    se, sc, sro = symmetric_part_arrays(*csr_of(s))
    d = _Device(s, 2 * s.nnz)
    count, msg = d.call(count_only=True)
    assert count == len(se) and not msg, msg
    runs = []
    for _ in range(2):
        got, msg = d.call()
        assert got == len(se) and not msg, msg
        runs.append(d.arrays(got))
    print(f"{name}: {s.Count} rows, {s.nnz} entries -> {count}")
    for e, c, ro in runs:
        assert np.array_equal(ro, sro) and np.array_equal(c, sc) and e.tobytes() == se.tobytes()
    d.dispose()
    # the Python routine is the same call
    P = amg.symmetric_part_gpu(s)
    assert np.array_equal(P.RowOffsets, sro) and np.array_equal(P.ColumnIndeces, sc) and P.Elements.tobytes() == se.tobytes()
    assert P.b.tobytes() == np.asarray(s.b, dtype=np.float64).tobytes() and P.grid == s.grid


def test_a_capacity_of_the_count_suffices_and_one_below_is_refused_with_the_output_untouched():
    s = PART["random1037"]()
    se, sc, sro = symmetric_part_arrays(*csr_of(s))
    d = _Device(s, len(se))
    got, msg = d.call(capacity=len(se) - 1)
    assert got == -1 and f"outCapacity {len(se) - 1} is below the {len(se)} entries" in msg, msg
    e, c, ro = d.arrays(len(se))
    assert np.all(e == 7.0) and np.all(c == -7) and np.all(ro == -7)
    got, msg = d.call()
    assert got == len(se) and not msg
    e, c, ro = d.arrays(got)
    assert np.array_equal(ro, sro) and np.array_equal(c, sc) and e.tobytes() == se.tobytes()
    d.dispose()


def test_a_column_out_of_range_is_refused():
    s = one_way_pair()
    s.ColumnIndeces[1] = 2
    d = _Device(s, 6)
    got, msg = d.call()
    assert got == -1 and "row 0 stores column 2" in msg, msg
    d.dispose()


# --------------------------------------------------------------------------- 2. the hierarchy of strength = 1
SYSTEMS = {
    "upwind20": lambda: upwind(20),
    "central16": lambda: central(16),
    "random3000": lambda: problems.random_nonsymmetric(3000),
}


@functools.lru_cache(maxsize=None)
def _system(name):
    return SYSTEMS[name]()


@functools.lru_cache(maxsize=None)
def _yardstick(name, passes):
    return HierarchySym(*csr_of(_system(name)), passes=passes)           # the defaults of ConjugateGradientAmgGpu


def _levels_of(H):
    return [(L["e"], L["c"], L["ro"], L["dinv"]) for L in H.levels]


@pytest.mark.parametrize("passes", [1, 3, 4])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_the_hierarchy_equals_the_yardstick_bit_for_bit(name, passes):
    s = _system(name)
    H = _yardstick(name, passes)
    cg = _amg(s, passes=passes, strength="symmetric")
    print(f"{name} passes {passes}: rows per level {rows_per_level(H)}")
    assert len(H.levels) >= 2, "the case must coarsen to test anything"
    assert _lib.lib().MgStrength(cg.mg) == 1
    _assert_equal_hierarchies(cg, _levels_of(H))
    for l, L in enumerate(H.levels[:-1]):
        assert np.array_equal(cg.level_aggregates(l), L["map"]), l
    r = np.random.default_rng(5).standard_normal(s.Count)
    if name == "random3000":                                   # coarse rows of 35 to 50 entries, no M-matrix: the default mode's tree sums have
        with tuning(dot_order=1):                              # no bound derived here, the fixed order is compared alone
            assert np.array_equal(cg.Apply(r), H.apply(r))
    else:
        _assert_apply_equals(cg, H, r, f"{name} passes {passes}")
    cg.Dispose()


def test_a_symmetric_matrix_gives_the_hierarchy_of_strength_0_in_every_array():
    s = problems.poisson(12, 10, 8)
    own, sym = _amg(s), _amg(s, strength="symmetric")
    L = _lib.lib()
    assert (L.MgStrength(own.mg), L.MgStrength(sym.mg)) == (0, 1)
    assert own.levels == sym.levels >= 3
    _assert_equal_hierarchies(sym, [own.level_csr(l) + (own.level_dinv(l),) for l in range(own.levels)])
    for l in range(own.levels - 1):
        assert np.array_equal(own.level_aggregates(l), sym.level_aggregates(l))
    own.Dispose()
    sym.Dispose()


def test_the_upwind_stencil_has_one_level_with_strength_0_and_four_with_strength_1():
    s = _system("upwind20")
    own, sym = _amg(s), _amg(s, strength="symmetric")
    L = _lib.lib()
    assert L.MgLevels(own.mg) == 1 and L.MgLevels(sym.mg) == 4
    assert [L.MgLevelRows(sym.mg, l) for l in range(4)] == [8000, 1251, 249, 105]
    own.Dispose()
    sym.Dispose()


def test_the_class_gives_the_c_calls_hierarchy():
    s = _system("central16")
    cg = _amg(s, strength="symmetric")
    L = _lib.lib()
    mg = L.MgSetupAggregationEx(cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, s.nnz, s.Count,
                                8, 3, 0.25, 64, 0.8, 1, 4, 0.5, 1)
    assert mg and not _lib.last_error()
    assert L.MgStrength(mg) == 1 and L.MgLevels(mg) == cg.levels >= 2
    for l in range(cg.levels):
        e, c, ro = cg.level_csr(l)
        assert (L.MgLevelRows(mg, l), L.MgLevelNnz(mg, l)) == (len(ro) - 1, len(e))
        e2, c2, ro2 = np.empty_like(e), np.empty_like(c), np.empty_like(ro)
        L.MgLevelCopyCsr(mg, l, _ptr(e2), _ptr(c2), _ptr(ro2))
        assert np.array_equal(ro2, ro) and np.array_equal(c2, c) and e2.tobytes() == e.tobytes()
        if l + 1 < cg.levels:
            m = np.empty(len(ro) - 1, dtype=np.int32)
            assert L.MgLevelCopyAggregates(mg, l, _ptr(m)) == 0 and np.array_equal(m, cg.level_aggregates(l))
    # strength = 0 through the new export is MgSetupAggregation
    mg0 = L.MgSetupAggregationEx(cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, s.nnz, s.Count,
                                 8, 3, 0.25, 64, 0.8, 1, 4, 0.5, 0)
    assert mg0 and L.MgStrength(mg0) == 0 and L.MgLevels(mg0) == len(Hierarchy(*csr_of(s)).levels) == 1
    L.MgDestroy(mg0)
    L.MgDestroy(mg)
    cg.Dispose()


# --------------------------------------------------------------------------- 3. the solvers behind it
def test_bicgstab_behind_the_hierarchy_equals_the_yardstick_bit_for_bit(dot_order):
    s = _randn(_system("upwind20"))
    H = _yardstick("upwind20", 3)
    ref = pbicgstab_oracle(s, H.apply, _lib.RULE_CSHARP, level(s))
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    cg = _amg(s, tol=level(s), rule=_lib.RULE_CSHARP, strength="symmetric")
    cg.SolveBicgstab(trace=True)
    cg.Read()
    got = dict(x=cg.x.copy(), r=cg.ReadResidual(), iteration=cg.Iteration, residual=cg.Residual, true_residual=cg.TrueResidual, status=cg.status,
               trace=cg.trace)
    print("bodies", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)
    cg.Dispose()


@pytest.mark.parametrize("orth", [1, 2])
def test_gmres_behind_the_hierarchy_equals_the_yardstick_bit_for_bit(dot_order, orth):
    s = _randn(_system("upwind20"))
    H = _yardstick("upwind20", 3)
    ref = fgmres_oracle(s, 9, orth, H.apply, _lib.RULE_CSHARP, level(s))
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    cg = _amg(s, tol=level(s), rule=_lib.RULE_CSHARP, strength="symmetric")
    got = finish(cg, 9, orth)
    print("steps", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)
    cg.Dispose()


def test_the_gauss_seidel_smoother_is_accepted_and_bicgstab_reaches_the_level():
    s = _randn(upwind(16))
    tol = level(s)
    cg = _amg(s, tol=tol, strength="symmetric", smoother="gs")
    L = _lib.lib()
    assert L.MgStrength(cg.mg) == 1 and L.MgSmoother(cg.mg) == 1 and cg.levels >= 2
    cg.SolveBicgstab()
    cg.Read()
    true = float(np.linalg.norm(s.b - s.to_scipy() @ cg.x))
    print(f"rows per level {[L.MgLevelRows(cg.mg, l) for l in range(cg.levels)]}, {cg.Iteration} bodies, |b - A x| / level = {true / tol:.4f}")
    assert cg.status == _lib.OK and true <= 1.001 * tol
    cg.Dispose()


def test_a_refused_strength_leaves_the_object_able_to_set_up_and_solve():
    s = _randn(upwind(16))
    tol = level(s)
    cg = _amg(s, tol=tol)
    L = _lib.lib()
    assert cg.levels == 1
    cg.strength = "both"
    with pytest.raises(_lib.MgcgError, match="strength 'both'"):
        cg.Setup()
    assert cg.mg and L.MgLevels(cg.mg) == 1                   # refused before anything was touched
    for bad in (-1, 2):
        L.MgcgClearLastError()
        mg = L.MgSetupAggregationEx(cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, s.nnz, s.Count,
                                    8, 3, 0.25, 64, 0.8, 1, 4, 0.5, bad)
        assert not mg and f"strength {bad}" in _lib.last_error()
        L.MgcgClearLastError()
    cg.strength = "symmetric"
    cg.Setup()
    assert cg.levels >= 2 and L.MgStrength(cg.mg) == 1
    cg.SolveBicgstab()
    cg.Read()
    assert cg.status == _lib.OK and float(np.linalg.norm(s.b - s.to_scipy() @ cg.x)) <= 1.001 * tol
    cg.Dispose()
