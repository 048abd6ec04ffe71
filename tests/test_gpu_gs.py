"""The multicolour Gauss-Seidel smoother of the aggregation V-cycle on the GPU (MgSetSmoother(mg, 1), ConjugateGradientAmgGpu(smoother="gs"),
ConjugateGradientSsorGpu) against its numpy statement ``GsHierarchy`` in tests/test_gs_host.py.

Colours are compared level by level; under dot_order = 1 M^-1 r, SolveMg, SolveMinresMg and SolveBicgstabMg are one fixed sequence of IEEE
operations and must EQUAL the yardstick (the solves: the existing numpy loops with ``GsHierarchy.apply`` as M^-1).  The sweeps sum in stored
order in every mode; in the default mode only the residual pass of a level of more than 20 entries a row may differ
(``_default_mode_bound``).  Every refusal is checked for its message and for the Jacobi bits of the hierarchy it leaves behind."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.ssor import ConjugateGradientSsorGpu
from tests.gpu_util import cap_inside_a_chunk, same_bits, same_under_every_chunking, tuning
from tests.test_amg_host import (Hierarchy, box_maps, csr_of, dominant_graph, graph_laplacian, irregular_maps, one_way, path_graph, rows_per_level, serial_dot)
from tests.test_bicgstab_host import MAX_IT as BICGSTAB_MAX_IT
from tests.test_bicgstab_mg_host import level, pbicgstab_oracle, system as bicgstab_system
from tests.test_gpu_amg import _assert_same_solve, _maxnz, _solve, _system
from tests.test_gpu_bicgstab_mg import assert_equal_runs as assert_equal_bicgstab_runs, result_of as bicgstab_result
from tests.test_gpu_pminres import _finish as finish_minres, assert_equal_runs as assert_equal_minres_runs
from tests.test_gs_host import GsHierarchy, banded
from tests.test_pminres_host import m_norm, pminres_oracle, psystem
from conjugategradient_amd.solver import ApplicationException

pytestmark = pytest.mark.gpu


def _gs(s, tol=1e-8, max_it=500, min_it=0, x0=None, smoother="gs", **kw):
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), min_it, max_it, tol, smoother=smoother, **kw).load(s)
    if x0 is not None:
        cg.x[:] = x0
    cg.Initialize()
    return cg


def _default_mode_bound(H):
    """The distance the default mode may put between M^-1 r and the yardstick, relative to max |z|.  The sweeps sum every row in stored
    order in every mode, so only the residual pass of a level of more than 20 entries a row on average (several lanes and a tree) can
    differ: nothing on a hierarchy without such a level with a map, else 3e-12, the bound of tests/test_gpu_amg.py
    (_assert_apply_equals: worked out there for every pass of the Jacobi cycle, of which this cycle re-associates fewer; the systems here
    share its premises)."""
    return 3e-12 if any(len(L["e"]) > 20 * (len(L["ro"]) - 1) for L in H.levels[:-1]) else 0.0


def _assert_gs_equals(cg, H, what, seed=5, default_mode=True):
    """Colours of every level and M^-1 r against the yardstick: EQUAL under dot_order = 1, within _default_mode_bound otherwise."""
    L = _lib.lib()
    assert L.MgSmoother(cg.mg) == 1 and cg.levels == len(H.levels)
    print(f"{what}: rows per level {rows_per_level(H)}, colours {H.colours()}, rounds {H.rounds}")
    for l, level_ in enumerate(H.levels):
        assert L.MgLevelColours(cg.mg, l) == len(level_["lists"]), l
        assert same_bits(cg.level_colours(l), level_["colour"]), l
    r = np.random.default_rng(seed).standard_normal(len(H.levels[0]["ro"]) - 1)
    zref = H.apply(r)
    with tuning(dot_order=1):
        z1 = cg.Apply(r)
    assert same_bits(z1, zref), what
    if default_mode:
        z0 = cg.Apply(r)
        distance, bound = float(np.abs(z0 - zref).max() / np.abs(zref).max()), _default_mode_bound(H)
        print(f"{what}: default mode max |z - yardstick| / max |yardstick| = {distance:.3e} (bound {bound:.3e})")
        assert distance <= bound, (what, distance, bound)


# --------------------------------------------------------------------------- 1. colours and the cycle = the yardstick
NAMES = ["poisson12-permuted", "graph10", "arrowhead1037", "reversed", "diagonal-first", "duplicates"]


@functools.lru_cache(maxsize=None)
def _yardstick(name, passes):
    return GsHierarchy(*csr_of(_system(name)), passes=passes)             # the defaults of ConjugateGradientAmgGpu: omega 0.8, nuCoarse 4


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_colours_and_cycle_equal_the_yardstick(name, passes, nu):
    """The systems of tests/test_gpu_amg.py and its stored-order variants: 4 lanes a row on arrowhead's levels (whose row of 322 entries
    takes 81 rounds of them), 8 on the stencils, 16 on their coarse levels; the levels of long rows are in section 2."""
    s = _system(name)
    H = _yardstick(name, passes)
    H.nu = nu
    assert len(H.levels) >= 2, "the case must coarsen to test anything"
    cg = _gs(s, passes=passes, nu=nu)
    _assert_gs_equals(cg, H, f"{name} passes {passes} nu {nu}")
    cg.Dispose()


def test_the_preconditioner_is_symmetric_for_every_omega_below_2():
    s = _system("graph10")
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal(s.Count), rng.standard_normal(s.Count)
    for omega in (1.0, 1.9):
        cg = _gs(s, omega=omega)
        a, b = float(u @ cg.Apply(v)), float(v @ cg.Apply(u))
        assert abs(a - b) <= 1e-12 * abs(a) and a == a
        assert float(u @ cg.Apply(u)) > 0.0
        cg.Dispose()


# --------------------------------------------------------------------------- 2. levels of long rows: several rounds of 16 lanes a row
def test_irregular_aggregates_with_long_coarse_rows_equal_the_yardstick():
    s = dominant_graph(10, 3)
    maps = irregular_maps(s.Count)
    H = GsHierarchy(*csr_of(s), maps=maps)                      # (within 64 colours: tests/test_gs_host.py)
    assert len(H.levels[1]["e"]) > 20 * (len(H.levels[1]["ro"]) - 1)
    for nu in (1, 2):
        H.nu = nu
        cg = _gs(s, nu=nu, aggregates=maps)
        _assert_gs_equals(cg, H, f"irregular maps nu {nu}")
        cg.Dispose()


def test_a_band_of_25_entries_a_row_equals_the_yardstick():
    """300 rows coupled to 12 rows either side: level 0 itself holds more than 20 entries a row and at least 13 colours."""
    s = banded(300, 12)
    assert s.nnz > 20 * s.Count
    cg = _gs(s)
    _assert_gs_equals(cg, GsHierarchy(*csr_of(s)), "banded, the library's aggregates")
    cg.Dispose()
    cg = _gs(s, aggregates=[], nuCoarse=2, omega=1.0)
    _assert_gs_equals(cg, GsHierarchy(*csr_of(s), maps=[], nuCoarse=2, omega=1.0), "banded, one level")
    cg.Dispose()


# --------------------------------------------------------------------------- 3. tiny matrices
@pytest.mark.parametrize("n,rows", [(1, [1]), (2, [2, 1]), (3, [3, 1]), (5, [5, 1])])
def test_tiny_matrices_colour_apply_and_solve(n, rows):
    s = problems.poisson(n, 1, 1)
    H = GsHierarchy(*csr_of(s), minCoarse=0)
    assert rows_per_level(H) == rows
    cg = _gs(s, minCoarse=0)
    _assert_gs_equals(cg, H, f"{n} row(s)")
    with tuning(dot_order=1):
        got = _solve(cg)
    assert got["status"] == _lib.OK and np.linalg.norm(s.b - s.to_scipy() @ got["x"]) < 2e-8
    _assert_same_solve(got, H.pcg(np.asarray(s.b), dot=serial_dot), f"{n} row(s)")
    cg.Dispose()


# --------------------------------------------------------------------------- 4. beyond one grid of lanes
LANES = 2048 * 256                # kMaxGrid * kBlock of csrc/common.hpp: the lanes of one launch of the sweep; a longer row list takes a second trip


def test_a_colour_list_longer_than_one_launch_takes_a_second_trip():
    """A path of 1.3 M rows, one level: the first colour of a path is a maximal independent set, about 0.43 of the rows."""
    s = path_graph(1300000, 5)
    H = GsHierarchy(*csr_of(s), maps=[], nuCoarse=2)
    longest = max(len(rows) for rows, _, _, _ in H.levels[0]["lists"])
    assert longest > LANES, longest
    cg = _gs(s, aggregates=[], nuCoarse=2)
    _assert_gs_equals(cg, H, "path of 1 300 000 rows", default_mode=False)
    cg.Dispose()


# --------------------------------------------------------------------------- 5. SolveMg, bit for bit
@functools.lru_cache(maxsize=None)
def _reference_solve(name, variant):
    s, H = _system(name), _yardstick(name, 3)
    H.nu = 1
    b = np.asarray(s.b)
    free = H.pcg(b, dot=serial_dot)
    if variant == "plain":
        return dict(), free
    if variant == "guess":
        x0 = np.random.default_rng(8).standard_normal(s.Count)
        return dict(x0=x0), H.pcg(b, x0=x0, dot=serial_dot)
    if variant == "min-iteration":
        min_it = free["iteration"] + 4
        return dict(min_it=min_it), H.pcg(b, dot=serial_dot, min_it=min_it)
    cap = cap_inside_a_chunk(0, free["iteration"])
    return dict(max_it=cap), H.pcg(b, dot=serial_dot, max_it=cap)


@pytest.mark.parametrize("variant", ["plain", "guess", "min-iteration", "cap"])
@pytest.mark.parametrize("name", ["poisson12-permuted", "graph10"])
def test_solve_equals_the_yardstick_loop_bit_for_bit(name, variant):
    how, ref = _reference_solve(name, variant)
    print(f"{name} {variant}: yardstick iteration {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == (_lib.MAXIT_EXCEEDED if variant == "cap" else _lib.OK)
    with tuning(dot_order=1):
        cg = _gs(_system(name), **how)
        got = _solve(cg)
        cg.Dispose()
    _assert_same_solve(got, ref, (name, variant))


@pytest.mark.parametrize("order", [0, 1])
def test_chunking_cannot_change_a_solve(order):
    s = _system("graph10")

    def run(max_it):
        cg = _gs(s, max_it=max_it)
        out = _solve(cg)
        cg.Dispose()
        return out

    free = same_under_every_chunking(lambda: run(500), order)
    assert free["status"] == _lib.OK and free["iteration"] > 8
    cap = cap_inside_a_chunk(0, free["iteration"])
    capped = same_under_every_chunking(lambda: run(cap), order)
    assert capped["status"] == _lib.MAXIT_EXCEEDED and capped["iteration"] == cap + 1
    if order == 1:
        _assert_same_solve(free, _reference_solve("graph10", "plain")[1], "check_every")
        _assert_same_solve(capped, _reference_solve("graph10", "cap")[1], "check_every, capped")
    else:
        assert np.linalg.norm(s.b - s.to_scipy() @ free["x"]) < 2e-8


# --------------------------------------------------------------------------- 6. one level, two sweeps: SSOR
@pytest.mark.parametrize("omega", [1.0, 1.5])
def test_the_one_level_form_is_ssor_preconditioned_cg(omega):
    s = _system("graph10")
    H = GsHierarchy(*csr_of(s), maps=[], nuCoarse=2, omega=omega)
    cg = ConjugateGradientSsorGpu(s.Count, _maxnz(s), 0, 500, 1e-8, omega=omega).load(s)
    cg.Initialize()
    assert cg.levels == 1 and cg.nuCoarse == 2 and cg.smoother == "gs"
    _assert_gs_equals(cg, H, f"SSOR({omega})")
    ref = H.pcg(np.asarray(s.b), dot=serial_dot)
    jacobi = Hierarchy(*csr_of(s), maps=[], nuCoarse=1, omega=1.0).pcg(np.asarray(s.b), dot=serial_dot)
    print(f"SSOR({omega}): iterations {ref['iteration']}, Jacobi CG {jacobi['iteration']}")
    assert ref["status"] == _lib.OK and ref["iteration"] < jacobi["iteration"]
    with tuning(dot_order=1):
        got = _solve(cg)
    _assert_same_solve(got, ref, f"SSOR({omega})")
    cg.Dispose()


# --------------------------------------------------------------------------- 7. MINRES and BiCGStab on such a hierarchy
@pytest.mark.parametrize("shift", [0.0, 5.0])
def test_minres_with_the_gs_cycle_equals_its_numpy_loop(shift):
    """graph12 of tests/test_pminres_host.py; shift 5 lies inside its spectrum (the smallest eigenvalues are 1e-3, 3.01, 3.22): A - 5 I is
    indefinite, M stays the cycle of A."""
    s = psystem("graph12")
    H = GsHierarchy(*csr_of(s))
    tol = 1e-8 * m_norm(H.apply, np.asarray(s.b))
    ref = pminres_oracle(s, shift, H.apply, _lib.RULE_CSHARP, tol, max_it=3000)
    print(f"shift {shift}: iterations {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    if shift:
        assert np.linalg.eigvalsh(s.to_scipy().toarray())[0] < shift
    with tuning(dot_order=1):
        cg = _gs(s, tol=tol, max_it=3000)
        got = finish_minres(cg, lambda: cg.SolveMinres(shift=shift, trace=True))
    assert_equal_minres_runs(got, ref)


@pytest.mark.parametrize("through", ["own", "hierarchy="])
def test_bicgstab_with_the_gs_cycle_equals_its_numpy_loop(through):
    """convection_diffusion(16, 16, 16, c = (.5, .25, 0)): nonsymmetric values on a symmetric pattern, box maps through MgSetupAggregates."""
    s = bicgstab_system("convdiff16")
    a = s.to_scipy()
    assert (a != a.T).nnz > 0 and ((a != 0) != (a != 0).T).nnz == 0
    maps = box_maps(s.grid, 3)
    H = GsHierarchy(*csr_of(s), maps=maps, omega=1.0)
    ref = pbicgstab_oracle(s, H.apply, _lib.RULE_CSHARP, level(s), max_it=BICGSTAB_MAX_IT)
    print(f"bodies {ref['iteration']}, status {ref['status']}")
    assert ref["status"] == _lib.OK and ref["iteration"] >= 3
    with tuning(dot_order=1):
        cg = _gs(s, tol=level(s), max_it=BICGSTAB_MAX_IT, aggregates=maps, omega=1.0, smoother="gs" if through == "own" else "jacobi")
        other = _gs(s, aggregates=maps, omega=1.0) if through != "own" else None
        try:
            cg.SolveBicgstab(trace=True, hierarchy=other)
        except ApplicationException:
            pass
        got = bicgstab_result(cg)
    cg.Dispose()
    if other is not None:
        other.Dispose()
    assert_equal_bicgstab_runs(got, ref)


# --------------------------------------------------------------------------- 8. refusals leave a usable Jacobi hierarchy
def _refused(cg, H, word):
    """MgSetSmoother(cg.mg, 1) is refused with `word` in its message; the hierarchy smooths with Jacobi as before, bit for bit."""
    L = _lib.lib()
    r = np.random.default_rng(5).standard_normal(cg.Count)
    with tuning(dot_order=1):
        before = cg.Apply(r)
        L.MgcgClearLastError()
        assert L.MgSetSmoother(cg.mg, 1) == -1
        msg = _lib.last_error()
        L.MgcgClearLastError()
        print(msg)
        assert "MgSetSmoother" in msg and word in msg, msg
        assert L.MgSmoother(cg.mg) == 0 and L.MgLevelColours(cg.mg, 0) == 0
        assert L.MgLevelCopyColours(cg.mg, 0, np.zeros(cg.Count, dtype=np.int32).ctypes.data) == -1 and "no colours" in _lib.last_error()
        L.MgcgClearLastError()
        after = cg.Apply(r)
    assert same_bits(before, after)
    if H is not None:
        assert same_bits(after, H.apply(r))
    return msg


def test_an_unsymmetric_pattern_is_refused():
    s = one_way(_system("graph10"))
    with pytest.raises(ValueError, match="level 0, row") as err:
        GsHierarchy(*csr_of(s))
    row = int(str(err.value).split("row ")[1])
    cg = _gs(s, smoother="jacobi")
    msg = _refused(cg, Hierarchy(*csr_of(s)), "not structurally symmetric")
    assert f"level 0, row {row}:" in msg                                     # the yardstick's row
    cg.Dispose()
    # the class: the library's message in MgcgError, a usable hierarchy behind it
    cg = ConjugateGradientAmgGpu(s.Count, _maxnz(s), 0, 500, 1e-8, smoother="gs").load(s)
    with pytest.raises(_lib.MgcgError, match=f"level 0, row {row}: .*not structurally symmetric"):
        cg.Initialize()
    assert cg.mg and _lib.lib().MgSmoother(cg.mg) == 0
    r = np.random.default_rng(5).standard_normal(s.Count)
    with tuning(dot_order=1):
        assert same_bits(cg.Apply(r), Hierarchy(*csr_of(s)).apply(r))
    cg.Dispose()


def test_a_geometric_hierarchy_is_refused():
    s = problems.poisson(8, 8, 4)
    geo = ConjugateGradientMgGpu(s.Count, 7, 0, 500, 1e-8, s.grid).load(s)
    geo.Initialize()
    _refused(geo, Hierarchy(*csr_of(s), omega=geo.omega, maps=box_maps(s.grid, 3)), "MgSetupAggregates")
    geo.Dispose()
    # ... and the same hierarchy from box maps takes the smoother
    cg = _gs(s, omega=6.0 / 7.0, aggregates=box_maps(s.grid, 3))
    _assert_gs_equals(cg, GsHierarchy(*csr_of(s), omega=6.0 / 7.0, maps=box_maps(s.grid, 3)), "box maps")
    cg.Dispose()


@pytest.mark.parametrize("nuCoarse", [1, 3])
def test_an_odd_coarse_count_is_refused(nuCoarse):
    s = _system("graph10")
    cg = _gs(s, smoother="jacobi", nuCoarse=nuCoarse)
    _refused(cg, Hierarchy(*csr_of(s), nuCoarse=nuCoarse), f"nuCoarse {nuCoarse}, must be even")
    cg.Dispose()


def test_more_than_64_colours_are_refused():
    s = problems.viennacl_main(n=300)
    with pytest.raises(ValueError, match="level 0, row") as err:
        GsHierarchy(*csr_of(s), maps=[])
    row = int(str(err.value).split("row ")[1])
    cg = _gs(s, smoother="jacobi")
    assert cg.levels == 1
    msg = _refused(cg, Hierarchy(*csr_of(s), maps=[]), "hold all 64 colours")
    assert f"level 0, row {row}:" in msg
    cg.Dispose()
    # the one-level class says the same
    cg = ConjugateGradientSsorGpu(s.Count, _maxnz(s), 0, 500, 1e-8).load(s)
    with pytest.raises(_lib.MgcgError, match=f"level 0, row {row}: .*hold all 64 colours"):
        cg.Initialize()
    cg.Dispose()


# --------------------------------------------------------------------------- 9. switching back and forth
def test_mode_0_restores_the_jacobi_bits_and_mode_1_twice_gives_the_same_bits():
    L = _lib.lib()
    s = _system("poisson12-permuted")
    J, G = Hierarchy(*csr_of(s)), _yardstick("poisson12-permuted", 3)
    G.nu = 1
    r = np.random.default_rng(5).standard_normal(s.Count)
    cg = _gs(s, smoother="jacobi")
    with tuning(dot_order=1):
        assert L.MgSmoother(cg.mg) == 0 and same_bits(cg.Apply(r), J.apply(r))
        seen = []
        for _ in range(2):
            assert L.MgSetSmoother(cg.mg, 1) == 0 and L.MgSmoother(cg.mg) == 1
            seen.append(([cg.level_colours(l) for l in range(cg.levels)], cg.Apply(r)))
        assert same_bits(seen[0][0], seen[1][0]) and same_bits(seen[0][1], seen[1][1]) and same_bits(seen[0][1], G.apply(r))
        assert L.MgSetSmoother(cg.mg, 0) == 0 and L.MgSmoother(cg.mg) == 0 and L.MgLevelColours(cg.mg, 0) == 0
        assert same_bits(cg.Apply(r), J.apply(r))
        got = _solve(cg)
    _assert_same_solve(got, J.pcg(np.asarray(s.b), dot=serial_dot), "Jacobi after Gauss-Seidel")
    cg.Dispose()
