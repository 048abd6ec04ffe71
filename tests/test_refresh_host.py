"""MgUpdateValues without a device: the numpy statement of the numeric refresh of an aggregation hierarchy -- the source lists of the
Galerkin products and the serial sums over them -- against the yardstick of tests/test_amg_host.py, the systems tests/test_gpu_refresh.py
runs on the GPU, and the library's refusals before any device call."""
import ctypes as C
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import (Hierarchy, _VectorHead, arrowhead, csr_of, diagonal_inverse, galerkin, graph_laplacian, irregular_maps,
                                 pairs_with_a_negative_coarse_diagonal, permuted, reversed_rows, rows_per_level, with_duplicates)


# --------------------------------------------------------------------------- the yardstick
def galerkin_sources(c, ro, amap, nc):
    """(sources, offsets) of sigma * P^T A P: the stored positions of A's entries grouped by coarse entry (coarse rows ascending, their
    columns ascending), inside a group in the contract's order -- members ascending, each member's entries in stored order.  A stable
    sort of the contract-order entry stream by coarse entry; offsets has one more entry than the coarse matrix has."""
    amap = np.asarray(amap, dtype=np.int64)
    ro = np.asarray(ro, dtype=np.int64)
    members = np.argsort(amap, kind="stable")
    length = np.diff(ro)[members]
    total = int(length.sum())
    first = np.cumsum(length) - length
    k = np.repeat(ro[:-1][members] - first, length) + np.arange(total)          # the stored entries in the contract's order
    key = np.repeat(amap[members], length) * nc + amap[np.asarray(c, dtype=np.int64)[k]]
    order = np.argsort(key, kind="stable")
    key = key[order]
    head = np.r_[True, key[1:] != key[:-1]] if total else np.zeros(0, dtype=bool)
    return k[order].astype(np.int32), np.r_[np.nonzero(head)[0], total].astype(np.int32)


def galerkin_numeric(e, sources, offsets, sigma):
    """C[q] = sigma * (((+0.0 + e[s0]) + e[s1]) + ...) over q's sources in list order."""
    offsets = np.asarray(offsets, dtype=np.int64)
    vals = np.asarray(e, dtype=np.float64)[sources]
    length = np.diff(offsets)
    acc = np.zeros(len(length))
    short = length <= 64
    for j in range(int(length[short].max()) if short.any() else 0):
        q = np.nonzero(short & (length > j))[0]
        acc[q] = acc[q] + vals[offsets[q] + j]
    for q in np.nonzero(~short)[0]:                                              # (accumulate adds strictly left to right)
        acc[q] = np.add.accumulate(np.r_[0.0, vals[offsets[q]:offsets[q + 1]]])[-1]
    return sigma * acc


def reversed_in_segments(sources, offsets):
    """The same lists with every segment back to front."""
    offsets = np.asarray(offsets, dtype=np.int64)
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    at = np.arange(len(sources))
    return sources[offsets[seg] + offsets[seg + 1] - 1 - at]


def refreshed(H, e):
    """The levels MgUpdateValues leaves from the hierarchy H (its patterns and maps) and level-0 values e, as a list of
    dict(e, c, ro, dinv, map, nc); ValueError "level l, row i" where a diagonal is not stored, finite and > 0."""
    out = []
    e = np.asarray(e, dtype=np.float64)
    for l, L in enumerate(H.levels):
        try:
            dinv = diagonal_inverse(e, L["c"], L["ro"])
        except ValueError as err:
            raise ValueError(f"level {l}, {err}") from None
        out.append(dict(L, e=e, dinv=dinv))
        if L["map"] is not None:
            e = galerkin_numeric(e, *galerkin_sources(L["c"], L["ro"], L["map"], L["nc"]), H.sigma)
    return out


# --------------------------------------------------------------------------- the systems (tests/test_gpu_refresh.py runs the same)
def with_values(s, e, name=None):
    """s's pattern, right-hand side and stored order with the values e."""
    return problems.LinearSystem(np.ascontiguousarray(e, dtype=np.float64), np.array(s.ColumnIndeces[: s.nnz], dtype=np.int32), np.array(s.RowOffsets, dtype=np.int32),
                                 np.zeros(s.Count), np.array(s.b, dtype=np.float64), name or s.name + "-new")


def scaled(s, seed=4):
    """D A D with d ~ U(0.5, 2) in s's stored order: symmetric positive definite where s is, the same pattern, other values."""
    e, c, ro = csr_of(s)
    d = np.random.default_rng(seed).uniform(0.5, 2.0, s.Count)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    return with_values(s, d[rows] * e * d[c])


def _graph():
    a, b = graph_laplacian(10, 3), graph_laplacian(10, 4)
    assert np.array_equal(a.ColumnIndeces, b.ColumnIndeces) and np.array_equal(a.RowOffsets, b.RowOffsets)
    return a, with_values(a, b.Elements[: b.nnz]), dict()


def _poisson(passes):
    a = permuted(problems.poisson(12, 12, 12), 7)
    return a, scaled(a), dict(passes=passes)


def _arrowhead(irregular):
    a = arrowhead()
    return a, scaled(a), dict(aggregates=irregular_maps(a.Count)) if irregular else dict()


BASES = {
    "graph10": _graph,
    "poisson12-passes1": lambda: _poisson(1),
    "poisson12-passes3": lambda: _poisson(3),
    "arrowhead-irregular": lambda: _arrowhead(True),
    "arrowhead-matching": lambda: _arrowhead(False),
}
ORDERS = {"stored": lambda s: s, "duplicates": with_duplicates, "reversed": reversed_rows}
CASES = [f"{base}-{order}" for base in BASES for order in ORDERS]


@functools.lru_cache(maxsize=None)
def case(name):
    """(first system, system of the new values, constructor keywords, yardstick of the first, its maps, yardstick of the new values built
    from those maps)."""
    base, order = name.rsplit("-", 1)
    a, b, kw = BASES[base]()
    a, b = ORDERS[order](a), ORDERS[order](b)
    assert np.array_equal(a.ColumnIndeces, b.ColumnIndeces) and np.array_equal(a.RowOffsets, b.RowOffsets) and not np.array_equal(a.Elements, b.Elements)
    H = Hierarchy(*csr_of(a), maps=kw.get("aggregates"), **{k: v for k, v in kw.items() if k != "aggregates"})
    maps = [L["map"] for L in H.levels[:-1]]
    return a, b, kw, H, maps, Hierarchy(*csr_of(b), maps=maps)


@pytest.mark.parametrize("name", CASES)
def test_the_numeric_pass_over_the_source_lists_equals_the_galerkin_product(name):
    a, b, _, H, maps, Hb = case(name)
    assert len(H.levels) >= 2 and rows_per_level(Hb) == rows_per_level(H)
    for L, Lb in zip(H.levels, Hb.levels):                                       # the maps are kept: so is every level's pattern
        assert np.array_equal(L["c"], Lb["c"]) and np.array_equal(L["ro"], Lb["ro"])
    order_shows = []
    for values, Hv in ((csr_of(b)[0], Hb), (csr_of(a)[0], H)):
        levels = refreshed(H, values)                                            # H's patterns and maps, other values
        assert len(levels) == len(Hv.levels)
        for l, (got, ref) in enumerate(zip(levels, Hv.levels)):
            assert got["e"].tobytes() == ref["e"].tobytes() and got["dinv"].tobytes() == ref["dinv"].tobytes(), (name, l)
    for l, L in enumerate(Hb.levels[:-1]):
        sources, offsets = galerkin_sources(L["c"], L["ro"], L["map"], L["nc"])
        e, c, ro = galerkin(L["e"], L["c"], L["ro"], L["map"], L["nc"], Hb.sigma)
        assert len(offsets) == len(e) + 1 and offsets[0] == 0 and offsets[-1] == len(L["e"]) and np.all(np.diff(offsets) >= 1)
        assert np.array_equal(np.sort(sources), np.arange(len(L["e"])))          # every fine entry once
        assert galerkin_numeric(L["e"], sources, offsets, Hb.sigma).tobytes() == e.tobytes() == Hb.levels[l + 1]["e"].tobytes()
        back = galerkin_numeric(L["e"], reversed_in_segments(sources, offsets), offsets, Hb.sigma)
        order_shows.append(float(np.mean(back != e)))
    print(f"{name}: rows per level {rows_per_level(H)}, entries that differ with every segment reversed, per level: {[f'{x:.1%}' for x in order_shows]}")
    assert max(order_shows) > 0, "the order of a sum does not show in these values: the case cannot tell a reordered sum"


def test_reversed_in_segments_reverses_every_segment():
    assert np.array_equal(reversed_in_segments(np.array([5, 6, 7, 1, 2, 9]), np.array([0, 3, 3, 5, 6])), [7, 6, 5, 2, 1, 9])


def test_the_sum_starts_from_plus_zero_and_keeps_zero_sums():
    e = np.array([-0.0, 1.5, -1.5, 2.0])
    got = galerkin_numeric(e, np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 1, 3, 4], dtype=np.int32), 0.5)
    assert got.tobytes() == np.array([0.0, 0.0, 1.0]).tobytes()                  # +0.0 + -0.0 = +0.0; the zero sum stays an entry
    long = np.random.default_rng(1).standard_normal(300)
    want = 0.0
    for v in long:
        want = want + v
    assert galerkin_numeric(long, np.arange(300, dtype=np.int32), np.array([0, 300], dtype=np.int32), 1.0)[0] == want


def test_a_coarse_diagonal_the_new_values_make_negative_is_refused_by_the_yardstick():
    bad = pairs_with_a_negative_coarse_diagonal()
    e = csr_of(bad)[0]
    rows = np.repeat(np.arange(bad.Count), np.diff(bad.RowOffsets))
    good = with_values(bad, np.where(bad.ColumnIndeces == rows, 3.0, e))
    H = Hierarchy(*csr_of(good), maps=[np.arange(200, dtype=np.int32) // 2])
    assert rows_per_level(H) == [200, 100]
    with pytest.raises(ValueError, match="level 1, row 0"):
        refreshed(H, e)
    broken = csr_of(good)[0].copy()
    broken[int(good.RowOffsets[37])] = np.nan                                     # (row 37's first stored entry is its diagonal or its neighbour's coupling)
    broken[int(good.RowOffsets[37]) + 1] = np.nan
    with pytest.raises(ValueError, match="level 0, row 37"):
        refreshed(H, broken)


# --------------------------------------------------------------------------- the library without a device
def test_exports_and_python_surface(hiplib):
    for name in ("MgUpdateValues", "MgUpdateBytes", "MgLevelCopyGalerkinSources"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    from conjugategradient_amd import amg, ssor

    for cls in (amg.ConjugateGradientAmgGpu, ssor.ConjugateGradientSsorGpu):
        for method in ("UpdateValues", "update_bytes", "level_galerkin_sources"):
            assert callable(getattr(cls, method))


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    """A zeroed handle is no aggregation hierarchy (and no ILU(0) factor): refused as a geometric one is.  The count and size refusals need
    an aggregation hierarchy, and there is none without a device: tests/test_gpu_refresh.py has them."""
    L = hiplib
    handle = C.create_string_buffer(4096)
    h = C.addressof(handle)
    big = _VectorHead(None, 28, -1, b"")
    vec = C.addressof(big)

    def message(call):
        L.MgcgClearLastError()
        status = call()
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return status, msg

    for mg, v in ((None, vec), (h, None), (None, None)):
        status, msg = message(lambda: L.MgUpdateValues(mg, v, 28))
        assert status == -1 and "MgUpdateValues: null argument" in msg, msg
    status, msg = message(lambda: L.MgUpdateValues(h, vec, 28))
    assert status == -1 and "MgUpdateValues: a geometric hierarchy" in msg and "MgSetup again" in msg, msg
    assert L.MgUpdateBytes(None) == 0 and L.MgUpdateBytes(h) == 0
    offsets, sources = (C.c_int * 4)(), (C.c_int * 4)()
    status, msg = message(lambda: L.MgLevelCopyGalerkinSources(None, 0, offsets, sources))
    assert status == -1 and "MgLevelCopyGalerkinSources: null handle" in msg, msg
    status, msg = message(lambda: L.MgLevelCopyGalerkinSources(h, 0, offsets, sources))
    assert status == -1 and "no aggregation hierarchy" in msg, msg
