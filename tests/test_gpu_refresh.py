"""MgUpdateValues on the GPU: new values for the pattern of an aggregation hierarchy, against the yardstick built from the kept maps
(tests/test_amg_host.py, tests/test_refresh_host.py) and against a second object set up by MgSetupAggregates from those maps.  Level
matrices, D^-1 and the source lists are compared bit for bit; M^-1 r and the solves under dot_order = 1, where every sum of the library
runs in the yardstick's order."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.ilu import ConjugateGradientIluGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.solver import ApplicationException
from conjugategradient_amd.ssor import ConjugateGradientSsorGpu
from tests.gpu_util import dvec, same_bits, tuning
from tests.test_amg_host import (Hierarchy, box_maps, csr_of, graph_laplacian, pairs_with_a_negative_coarse_diagonal, path_graph, permuted,
                                 rows_per_level, serial_dot, zero_before_the_diagonal)
from tests.test_amg_sym_host import upwind
from tests.test_gs_host import GsHierarchy
from tests.test_kcycle_host import KHierarchy
from tests.test_refresh_host import CASES, case, galerkin_sources, refreshed, scaled, with_values

pytestmark = pytest.mark.gpu

LANES = 2048 * 256                # kMaxGrid * kBlock of csrc/common.hpp: the lanes of one launch
TILE = 2048                       # kRefreshTile: the sources a workgroup stages in LDS at a time


def _maxnz(s):
    return int(np.diff(s.RowOffsets).max())


def _amg(s, cls=ConjugateGradientAmgGpu, compression=None, max_it=500, **kw):
    cg = cls(s.Count, _maxnz(s), 0, max_it, 1e-8, **kw).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    return cg


def _values(s):
    return np.array(s.Elements[: s.nnz], dtype=np.float64)


def _update(cg, e, form, parked):
    """UpdateValues in place, or MgUpdateValues with ANOTHER vector that then takes vectorA's place in the object (the solvers multiply by
    the vectors they are given); the vector it replaces is parked, alive, for the caller to dispose of."""
    if form == "in-place":
        cg.UpdateValues(e)
        return
    other = dvec(e)
    status = _lib.lib().MgUpdateValues(cg.mg, other.Ptr, len(e))
    try:
        _lib.check("MgUpdateValues")
        assert status == 0
    except _lib.MgcgError:
        other.Dispose()
        raise
    parked.append(cg.vectorA)
    cg.vectorA = other
    cg.A.Elements = np.array(e, dtype=np.float64)


def _solve(cg, how="Solve"):
    """One solve from x = 0 -> dict(status, iteration, residual, trace, x); the cap is a result here, not an exception."""
    cg.vectorX.CopyFrom(np.zeros(cg.Count), cg.Count)
    try:
        getattr(cg, how)(trace=True)
    except ApplicationException:
        assert cg.status == _lib.MAXIT_EXCEEDED
    cg.Read()
    return dict(status=cg.status, iteration=cg.Iteration, residual=cg.Residual, trace=cg.trace.copy(), x=cg.x.copy())


def _levels(cg):
    return [cg.level_csr(l) + (cg.level_dinv(l),) for l in range(cg.levels)]


def _levels_of(H):
    return [(L["e"], L["c"], L["ro"], L["dinv"]) for L in (H.levels if hasattr(H, "levels") else H)]


def _probe(n):
    return np.random.default_rng(5).standard_normal(n)


def _assert_levels(cg, H, what):
    ref = _levels_of(H)
    assert cg.levels == len(ref), what
    for l, (got, want) in enumerate(zip(_levels(cg), ref)):
        assert same_bits(got[0], want[0]), (what, l, "values")
        assert same_bits(got[3], want[3]), (what, l, "D^-1")
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, l, "pattern")


def _assert_is(cg, H, b, what, solve=True):
    """Levels, D^-1, M^-1 r and -- with `solve` -- SolveMg's trace and x against the yardstick H; call under dot_order = 1."""
    _assert_levels(cg, H, what)
    assert same_bits(cg.Apply(_probe(cg.Count)), H.apply(_probe(cg.Count))), (what, "M^-1 r")
    if solve:
        got, ref = _solve(cg), _reference_solve(H, b)
        assert (got["status"], got["iteration"], got["residual"]) == (ref["status"], ref["iteration"], ref["residual"]), what
        assert same_bits(got["trace"], ref["trace"]) and same_bits(got["x"], ref["x"]), what


_solves = {}


def _reference_solve(H, b):
    if id(H) not in _solves:
        _solves[id(H)] = (H, H.pcg(np.asarray(b, dtype=np.float64), dot=serial_dot))       # (H kept alive: its id stays its own)
    return _solves[id(H)][1]


def _with_levels(H, levels):
    out = copy.copy(H)
    out.levels = levels
    return out


# --------------------------------------------------------------------------- 1. equality with a fresh set-up from the same maps
@pytest.mark.parametrize("form", ["in-place", "other-vector"])
@pytest.mark.parametrize("name", CASES + ["poisson12-irregular"])
def test_a_refresh_equals_a_fresh_set_up_from_the_kept_maps(name, form):
    if name == "poisson12-irregular":
        a, b, kw, Ha, maps, Hb = _irregular()
    else:
        a, b, kw, Ha, maps, Hb = case(name)
    parked = []
    with tuning(dot_order=1):
        cg = _amg(a, **kw)
        assert cg.update_bytes() == 0
        with pytest.raises(_lib.MgcgError, match="first MgUpdateValues"):
            cg.level_galerkin_sources(0)
        _assert_is(cg, Ha, a.b, f"{name}: set-up")
        assert all(np.array_equal(cg.level_aggregates(l), m) for l, m in enumerate(maps))
        _update(cg, _values(b), form, parked)
        _assert_is(cg, Hb, b.b, f"{name} {form}: refreshed")
        assert all(np.array_equal(cg.level_aggregates(l), m) for l, m in enumerate(maps))
        for l, L in enumerate(Hb.levels[:-1]):
            sources, offsets = cg.level_galerkin_sources(l)
            want = galerkin_sources(L["c"], L["ro"], L["map"], L["nc"])
            assert same_bits(sources, want[0]) and same_bits(offsets, want[1]), (name, l)
        with pytest.raises(_lib.MgcgError, match="forms no next level"):
            cg.level_galerkin_sources(cg.levels - 1)
        twin = _amg(b, aggregates=[cg.level_aggregates(l) for l in range(cg.levels - 1)])
        assert same_bits(_levels(cg), _levels(twin)) and same_bits(cg.Apply(_probe(a.Count)), twin.Apply(_probe(a.Count)))
        twin.Dispose()
        _update(cg, _values(a), form, parked)
        _assert_is(cg, Ha, a.b, f"{name} {form}: refreshed back")
    for v in parked:
        v.Dispose()
    cg.Dispose()


@functools.lru_cache(maxsize=None)
def _irregular():
    """The caller's maps on the permuted 12^3 grid: aggregates of 1 .. 40 scattered rows, ids in no order, long coarse rows."""
    from tests.test_amg_host import irregular_maps

    a = permuted(problems.poisson(12, 12, 12), 7)
    b = scaled(a)
    maps = irregular_maps(a.Count)
    return a, b, dict(aggregates=maps), Hierarchy(*csr_of(a), maps=maps), maps, Hierarchy(*csr_of(b), maps=maps)


# --------------------------------------------------------------------------- 2. long segments
def test_one_aggregate_of_everything_is_one_segment_of_every_entry():
    a = permuted(problems.poisson(12, 12, 12), 7)
    b = scaled(a)
    maps = [np.zeros(a.Count, dtype=np.int32)]
    assert a.nnz == 11232 > 5 * TILE
    Ha, Hb = Hierarchy(*csr_of(a), maps=maps), Hierarchy(*csr_of(b), maps=maps)
    with tuning(dot_order=1):
        cg = _amg(a, aggregates=maps)
        cg.UpdateValues(_values(b))
        _assert_is(cg, Hb, b.b, "one aggregate")
        sources, offsets = cg.level_galerkin_sources(0)
        assert same_bits(offsets, np.array([0, a.nnz], dtype=np.int32)) and same_bits(sources, np.arange(a.nnz, dtype=np.int32))
        cg.UpdateValues(_values(a))
        _assert_is(cg, Ha, a.b, "one aggregate, back")
    cg.Dispose()


@functools.lru_cache(maxsize=None)
def _long_segment_path():
    n, head = 70001, 60000
    a = path_graph(n, 5, decades=2.0)
    b = with_values(a, _values(path_graph(n, 6, decades=2.0)))
    i = np.arange(n)
    maps = [np.where(i < head, 0, 1 + (i - head) // 2).astype(np.int32)]
    Ha = Hierarchy(*csr_of(a), maps=maps)
    return a, b, maps, Ha, _with_levels(Ha, refreshed(Ha, _values(b)))


def test_a_segment_longer_than_any_tile_continues_from_global_memory():
    """A path of 70 001 rows whose first 60 000 are ONE aggregate, pairs behind it: coarse entry (0, 0) sums 179 998 fine entries, 88 tiles
    of the list, next to segments of one to four.  Weights over two decades more: the order of that sum shows."""
    a, b, maps, Ha, Hb = _long_segment_path()
    lengths = np.diff(galerkin_sources(Ha.levels[0]["c"], Ha.levels[0]["ro"], maps[0], Ha.levels[0]["nc"])[1])
    assert lengths[0] == 3 * 60000 - 2 > 80 * TILE and lengths[1:].max() <= 4
    with tuning(dot_order=1):
        cg = _amg(a, aggregates=maps)
        _assert_levels(cg, Ha, "long segment: set-up")
        cg.UpdateValues(_values(b))
        _assert_is(cg, Hb, b.b, "long segment", solve=False)
        sources, offsets = cg.level_galerkin_sources(0)
        want = galerkin_sources(Ha.levels[0]["c"], Ha.levels[0]["ro"], maps[0], Ha.levels[0]["nc"])
        assert same_bits(sources, want[0]) and same_bits(offsets, want[1])
        twin = _amg(b, aggregates=maps)
        assert same_bits(_levels(cg), _levels(twin))
        twin.Dispose()
    cg.Dispose()


# --------------------------------------------------------------------------- 3. beyond one grid of lanes
def test_every_stride_loop_of_the_refresh_takes_a_second_trip():
    """The path of 2 * 2048 * 256 + 1077 rows, one pass a level: the sources of level 0 (3.1 M), its segments and the coarse entries (1.8 M)
    and the coarse rows (0.6 M) all exceed the lanes of one launch, in the list build and in the numeric pass.  (The numeric pass strides
    over TILES, 1538 here for 2048 workgroups: the test below has more.)"""
    from tests.test_gpu_amg import _long_path           # (the yardstick of its own second-trip test: built once a session)

    a, Ha = _long_path("uniform")
    b = with_values(a, _values(path_graph(a.Count, 6)))
    rows = rows_per_level(Ha)
    assert len(rows) == 3 and rows[1] > LANES and len(Ha.levels[1]["e"]) > LANES and a.nnz > LANES
    Hb = _with_levels(Ha, refreshed(Ha, _values(b)))
    cg = _amg(a, levels=3, passes=1)
    cg.UpdateValues(_values(b))
    with tuning(dot_order=1):
        _assert_is(cg, Hb, b.b, "second trips", solve=False)
    for l in (0, 1):
        L = Ha.levels[l]
        sources, offsets = cg.level_galerkin_sources(l)
        want = galerkin_sources(L["c"], L["ro"], L["map"], L["nc"])
        assert same_bits(sources, want[0]) and same_bits(offsets, want[1]), l
    cg.Dispose()


def test_the_numeric_pass_takes_a_second_trip_over_its_tiles():
    """The same path with every off-diagonal entry stored as two entries and a stored zero behind every diagonal: 6.3 M sources are more tiles of 2048 than a launch has workgroups (2048),
    so a workgroup of the numeric pass comes round to a second tile.  Two levels; against the numpy statement of the lists and the sums on
    the library's own map, and the diagonal rule of the set-up."""
    from tests.test_amg_host import diagonal_inverse, with_duplicates
    from tests.test_gpu_amg import _long_path
    from tests.test_refresh_host import galerkin_numeric

    s = _long_path("uniform")[0]
    a = with_duplicates(s)
    b = with_duplicates(with_values(s, _values(path_graph(s.Count, 6))))
    assert a.nnz > 2048 * TILE and np.array_equal(a.ColumnIndeces, b.ColumnIndeces)
    cg = _amg(a, levels=2, passes=1)
    assert cg.levels == 2
    amap = cg.level_aggregates(0)
    cg.UpdateValues(_values(b))
    e, c, ro = csr_of(b)
    sources, offsets = cg.level_galerkin_sources(0)
    want = galerkin_sources(c, ro, amap, int(amap.max()) + 1)
    assert same_bits(sources, want[0]) and same_bits(offsets, want[1])
    e1, c1, ro1 = cg.level_csr(1)
    assert len(e1) + 1 == len(offsets) and same_bits(e1, galerkin_numeric(e, sources, offsets, 0.5))
    assert same_bits(cg.level_csr(0)[0], e) and same_bits(cg.level_dinv(0), diagonal_inverse(e, c, ro)) and same_bits(cg.level_dinv(1), diagonal_inverse(e1, c1, ro1))
    cg.Dispose()


# --------------------------------------------------------------------------- 4. every mode keeps working
def test_the_gauss_seidel_smoother_keeps_its_colours_and_takes_the_new_values():
    a, b, kw, _, maps, _ = case("graph10-stored")
    Gb = GsHierarchy(*csr_of(b), maps=maps)
    with tuning(dot_order=1):
        cg = _amg(a, smoother="gs", **kw)
        colours = [cg.level_colours(l) for l in range(cg.levels)]
        cg.UpdateValues(_values(b))
        _assert_is(cg, Gb, b.b, "gs", solve=False)
        assert same_bits(colours, [cg.level_colours(l) for l in range(cg.levels)])
        assert all(np.array_equal(c, L["colour"]) for c, L in zip(colours, Gb.levels))
        got = _solve(cg)
        assert got["status"] == _lib.OK and np.linalg.norm(b.b - b.to_scipy() @ got["x"]) < 2e-8
    cg.Dispose()


@pytest.mark.parametrize("inner", ["conjugate", "minimal"])
def test_the_k_cycle_takes_the_new_values(inner):
    a, b, kw, _, maps, Hb = case("poisson12-passes3-stored")
    assert len(Hb.levels) >= 3
    Kb = KHierarchy.of(Hb, cycle="K", inner={"conjugate": 0, "minimal": 1}[inner], dot=serial_dot)
    with tuning(dot_order=1):
        cg = _amg(a, cycle="K", inner=inner, **kw)
        cg.UpdateValues(_values(b))
        _assert_is(cg, Kb, b.b, f"K-cycle, {inner}", solve=False)
        assert _lib.lib().MgCycle(cg.mg) == 1
        got = _solve(cg)
        assert got["status"] == _lib.OK and np.linalg.norm(b.b - b.to_scipy() @ got["x"]) < 2e-8
    cg.Dispose()


def test_the_symmetric_strength_hierarchy_of_an_upwind_stencil_takes_the_new_values():
    """10^3 upwind convection-diffusion, strength "symmetric"; the new values are D A D (nonsymmetric as A is).  Against the yardstick from
    the kept maps and against a twin object set up from them: levels, M^-1 r, SolveBicgstab and SolveGmres, bit for bit."""
    a = upwind(10)
    b = scaled(a)
    with tuning(dot_order=1):
        cg = _amg(a, strength="symmetric")
        assert cg.levels >= 2 and _lib.lib().MgStrength(cg.mg) == 1
        maps = [cg.level_aggregates(l) for l in range(cg.levels - 1)]
        cg.UpdateValues(_values(b))
        _assert_is(cg, Hierarchy(*csr_of(b), maps=maps), b.b, "upwind", solve=False)
        twin = _amg(b, aggregates=maps)
        for how in ("SolveBicgstab", "SolveGmres"):
            got, ref = _solve(cg, how), _solve(twin, how)
            assert got["status"] == ref["status"] == _lib.OK and got["iteration"] == ref["iteration"] and got["residual"] == ref["residual"], how
            assert same_bits(got["trace"], ref["trace"]) and same_bits(got["x"], ref["x"]), how
            assert np.linalg.norm(b.b - b.to_scipy() @ got["x"]) < 1e-6 * np.linalg.norm(b.b), how
        twin.Dispose()
    cg.Dispose()


def test_a_hierarchy_of_one_level_gets_its_new_diagonal():
    a = problems.viennacl_main(n=2000)
    b = scaled(a)
    Hb = Hierarchy(*csr_of(b))
    assert len(Hb.levels) == 1
    with tuning(dot_order=1):
        cg = _amg(a, max_it=2000)
        assert cg.levels == 1
        cg.UpdateValues(_values(b))
        _assert_is(cg, Hb, b.b, "one level", solve=False)
        assert cg.update_bytes() > 0
        cg.Dispose()
        # ... and the SSOR class, one level of two Gauss-Seidel sweeps, through inheritance
        a, b = case("graph10-stored")[:2]
        Gb = GsHierarchy(*csr_of(b), maps=[], omega=1.0, nuCoarse=2)
        cg = _amg(a, cls=ConjugateGradientSsorGpu)
        cg.UpdateValues(_values(b))
        _assert_is(cg, Gb, b.b, "SSOR", solve=False)
    cg.Dispose()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_matrices_refresh(n):
    a = problems.poisson(n, 1, 1)
    b = scaled(a)
    Ha = Hierarchy(*csr_of(a), minCoarse=0)
    Hb = Hierarchy(*csr_of(b), maps=[L["map"] for L in Ha.levels[:-1]], minCoarse=0)
    with tuning(dot_order=1):
        cg = _amg(a, minCoarse=0)
        cg.UpdateValues(_values(b))
        _assert_is(cg, Hb, b.b, f"{n} row(s)")
        cg.UpdateValues(_values(a))
        _assert_is(cg, Ha, a.b, f"{n} row(s), back")
    cg.Dispose()


# --------------------------------------------------------------------------- 5. the analysis cache
def _classes(cg):
    """The class of every analysis the handle holds (MgcgAnalysisInfo): 0 = plain CSR kept, 1 .. 5 = a lossless form in use."""
    L, out = _lib.lib(), []
    while L.MgcgAnalysisInfo(cg.cusparse, len(out), None, None, None, None) >= 0:
        out.append(L.MgcgAnalysisInfo(cg.cusparse, len(out), None, None, None, None))
    return out


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_compressed_forms_are_those_of_the_new_values(mode):
    """a -> b -> a -> b on one handle with the analysis cache on: the shadow buffers come round again at the same addresses, and every
    level's form must be that of the values in force."""
    a, b, kw, Ha, _, Hb = case("graph10-stored")
    with tuning(dot_order=1):
        cg = _amg(a, compression=mode, **kw)
        _assert_is(cg, Ha, a.b, f"mode {mode}: set-up")
        for turn, (s, H) in enumerate(((b, Hb), (a, Ha), (b, Hb))):
            cg.UpdateValues(_values(s))
            _assert_is(cg, H, s.b, f"mode {mode}, turn {turn}")
            assert max(_classes(cg)) >= 1, "no level took a compressed form: there is no analysis that could be stale"
    cg.Dispose()


# --------------------------------------------------------------------------- 6. refusals and what follows
def _with_diagonal(s, row, value):
    e = _values(s)
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    e[(rows == row) & (np.asarray(s.ColumnIndeces[: s.nnz]) == rows)] = value
    return e


@functools.lru_cache(maxsize=None)
def _refusal_base(kind):
    """(good system, bad values of its pattern, maps, yardstick).  zero-first: the pattern holds column 37 twice in row 37; the FIRST stored
    one is the diagonal -- 6 then 0 in the good values, 0 then 6 in the bad ones."""
    s = problems.poisson(8, 8, 4)
    if kind == "zero-first":
        z = zero_before_the_diagonal(s, 37)
        at = int(z.RowOffsets[37])
        rows = np.repeat(np.arange(z.Count), np.diff(z.RowOffsets))
        second = np.nonzero((rows == 37) & (z.ColumnIndeces[: z.nnz] == 37))[0][1]
        bad = _values(z)
        assert bad[at] == 0.0 and bad[second] == 6.0
        good = bad.copy()
        good[at], good[second] = 6.0, 0.0
        s = with_values(z, good)
    else:
        bad = _with_diagonal(s, 37, {"negative": -6.0, "nan": np.nan, "infinite": np.inf}[kind])
    maps = box_maps((8, 8, 4), 2)
    return s, bad, maps, Hierarchy(*csr_of(s), maps=maps)


@pytest.mark.parametrize("form", ["in-place", "other-vector"])
@pytest.mark.parametrize("kind", ["zero-first", "negative", "nan", "infinite"])
def test_a_bad_diagonal_on_level_0_is_refused_and_nothing_changes(kind, form):
    s, bad, maps, H = _refusal_base(kind)
    parked = []
    with tuning(dot_order=1):
        cg = _amg(s, aggregates=maps)
        for turn in (0, 1):                              # before the lists exist, and with them
            with pytest.raises(_lib.MgcgError, match="MgUpdateValues: level 0, row 37: the diagonal must be stored, finite and > 0"):
                _update(cg, bad, form, parked)
            if form == "other-vector":
                _assert_is(cg, H, s.b, f"{kind}: after the refusal", solve=False)
            else:                                        # level 0 is what the caller wrote, over the old coarse levels and the old D^-1
                got, ref = _levels(cg), _levels_of(H)
                assert same_bits(got[0][0], bad) and same_bits(got[0][3], ref[0][3])
                assert all(same_bits(g[0], r[0]) and same_bits(g[3], r[3]) for g, r in zip(got[1:], ref[1:]))
            _update(cg, _values(s), form, parked)
            _assert_is(cg, H, s.b, f"{kind}: a good refresh after the refusal")
    for v in parked:
        v.Dispose()
    cg.Dispose()


@pytest.mark.parametrize("form", ["in-place", "other-vector"])
def test_a_coarse_diagonal_the_new_values_make_negative_is_refused(form):
    bad = pairs_with_a_negative_coarse_diagonal()
    good = with_values(bad, _values(bad))
    rows = np.repeat(np.arange(bad.Count), np.diff(bad.RowOffsets))
    good.Elements[good.ColumnIndeces == rows] = 3.0
    maps = [np.arange(200, dtype=np.int32) // 2]
    H = Hierarchy(*csr_of(good), maps=maps)
    parked = []
    with tuning(dot_order=1):
        cg = _amg(good, aggregates=maps)
        with pytest.raises(_lib.MgcgError, match="MgUpdateValues: level 1, row 0: the diagonal"):
            _update(cg, _values(bad), form, parked)
        if form == "other-vector":
            _assert_is(cg, H, good.b, "pairs: after the refusal", solve=False)
        else:
            assert same_bits(cg.level_csr(1)[0], H.levels[1]["e"]) and same_bits(cg.level_dinv(0), H.levels[0]["dinv"])
        _update(cg, _values(good), form, parked)
        _assert_is(cg, H, good.b, "pairs: a good refresh after the refusal")
    for v in parked:
        v.Dispose()
    cg.Dispose()


def test_other_handles_and_bad_arguments_are_refused_and_the_handles_stay_as_they_were():
    L = _lib.lib()
    s = problems.poisson(8, 8, 8)
    r = _probe(s.Count)

    def refused(call, message):
        L.MgcgClearLastError()
        status = call()
        msg = _lib.last_error()
        L.MgcgClearLastError()
        assert status == -1 and message in msg, msg

    geo = ConjugateGradientMgGpu(s.Count, 7, 0, 500, 1e-8, s.grid).load(s)
    geo.Initialize()
    ilu = _amg(s, cls=ConjugateGradientIluGpu)
    for cg, message in ((geo, "a geometric hierarchy has no numeric refresh, call MgSetup again"), (ilu, "the handle is an ILU(0) factor: it has no numeric refresh, call MgSetupIlu0 again")):
        before = cg.Apply(r)
        refused(lambda: L.MgUpdateValues(cg.mg, cg.vectorA.Ptr, s.nnz), "MgUpdateValues: " + message)
        assert L.MgUpdateBytes(cg.mg) == 0
        refused(lambda: L.MgLevelCopyGalerkinSources(cg.mg, 0, None, None), "no aggregation hierarchy")
        assert same_bits(cg.Apply(r), before)
        cg.Dispose()
    cg = _amg(s)
    before = _levels(cg), cg.Apply(r)
    short = dvec(np.ones(s.nnz - 1))
    refused(lambda: L.MgUpdateValues(cg.mg, cg.vectorA.Ptr, s.nnz - 1), f"elementsCount {s.nnz - 1}, the hierarchy was built from {s.nnz} entries")
    refused(lambda: L.MgUpdateValues(cg.mg, short.Ptr, s.nnz), f"the vector holds {s.nnz - 1} values")
    refused(lambda: L.MgUpdateValues(cg.mg, None, s.nnz), "null argument")
    with pytest.raises(_lib.MgcgError, match="UpdateValues: 5 values"):
        cg.UpdateValues(np.ones(5))
    assert cg.update_bytes() == 0 and same_bits((_levels(cg), cg.Apply(r)), before)
    short.Dispose()
    cg.Dispose()


# --------------------------------------------------------------------------- 7. lists built once
def test_the_lists_are_built_once_and_a_refresh_is_reproducible():
    a, b, kw, _, _, Hb = case("poisson12-passes3-stored")
    cg = _amg(a, **kw)
    assert cg.update_bytes() == 0
    cg.UpdateValues(_values(b))
    first = cg.update_bytes()
    lists = 4 * sum(len(L["e"]) + len(M["e"]) + 1 for L, M in zip(Hb.levels[:-1], Hb.levels[1:]))
    shadows = 8 * (sum(len(L["e"]) for L in Hb.levels[1:]) + sum(rows_per_level(Hb)))
    print(f"update_bytes {first}: lists {lists}, shadow buffers {shadows}, flags {16 * cg.levels}")
    assert first == lists + shadows + 16 * cg.levels
    one = _levels(cg), cg.Apply(_probe(a.Count))
    cg.UpdateValues(None)                                # the device vector as it stands: the same values again
    assert cg.update_bytes() == first
    assert same_bits((_levels(cg), cg.Apply(_probe(a.Count))), one)
    cg.UpdateValues(_values(b))
    assert cg.update_bytes() == first and same_bits((_levels(cg), cg.Apply(_probe(a.Count))), one)
    _assert_levels(cg, Hb, "twice")
    cg.Dispose()
