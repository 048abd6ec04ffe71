"""CSR transposition on the device (MgcgCsrTranspose) against its numpy yardstick in tests/test_transpose_host.py -- offsets, columns, value
bytes and source list, in two calls of every case -- on every path of kernels_transpose.hip: the three width classes of the segment sort
and both sides of their boundaries, grid-stride loops that take a second trip, empty rows and columns, duplicates, unsorted rows; the
refusals made once the arrays have been read; and MgcgSymmetricPart / MgSetupAggregationEx(strength = 1), which are built on it, on columns
long enough to leave the register class.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, amg, problems
from conjugategradient_amd.solver import ConjugateGradientGpu
from tests.gpu_util import dvec, ivec
from tests.test_amg_host import _raw, csr_of, reversed_rows, rows_per_level, with_duplicates
from tests.test_amg_sym_host import HierarchySym, NONSYMMETRIC, symmetric_part_arrays
from tests.test_gpu_amg import _assert_equal_hierarchies
from tests.test_gpu_amg_sym import _Device as _PartDevice, _amg, _levels_of
from tests.test_transpose_host import arrow_fast, transpose_arrays

pytestmark = pytest.mark.gpu

SHORT_MAX, LDS_MAX = amg.transpose_class_limits()
LANES = 2048 * 256                                            # kMaxGrid * kBlock: more entries or columns than this and a grid-stride loop takes a second trip


class _Device:
    """CSR arrays in device vectors of the library, the two handles, and output vectors of `held` entries filled with 7.0 / -7."""

    def __init__(self, e, c, ro, columns, held=None, source=True):
        self.rows, self.columns, self.held = len(ro) - 1, columns, len(c) if held is None else held
        self.blas, self.sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
        room = max(self.held, 1)
        self.a = None if e is None else dvec(e)
        self.ro, self.ci = ivec(ro), ivec(c)
        self.ta = None if e is None else dvec(np.full(room, 7.0))
        self.tro, self.tci = ivec(np.full(columns + 1, -7)), ivec(np.full(room, -7))
        self.src = ivec(np.full(room, -7)) if source else None

    def call(self):
        L = _lib.lib()
        L.MgcgClearLastError()
        ptr = lambda v: None if v is None else v.Ptr
        got = L.MgcgCsrTranspose(self.blas, self.sparse, ptr(self.a), self.ro.Ptr, self.ci.Ptr, self.held, self.rows, self.columns,
                                 ptr(self.ta), self.tro.Ptr, self.tci.Ptr, ptr(self.src))
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return got, msg

    def arrays(self):
        """(elements, columns, offsets, source) in their whole length (None where the vector was not given)"""
        room = max(self.held, 1)
        return (None if self.ta is None else self.ta.to_numpy(room), self.tci.to_numpy(room), self.tro.to_numpy(self.columns + 1),
                None if self.src is None else self.src.to_numpy(room))

    def dispose(self):
        for v in (self.a, self.ro, self.ci, self.ta, self.tro, self.tci, self.src):
            if v is not None:
                v.Dispose()
        _lib.lib().DestroyBlas(self.blas)
        _lib.lib().DestroySparse(self.sparse)


def _assert_transposes(e, c, ro, columns, held=None, source=True):
    """Two calls, each equal to the yardstick in every array; what lies beyond the result keeps its fill.  Returns the device's arrays."""
    we, wc, wro, wsrc = transpose_arrays(e, c, ro, columns)
    nnz = int(np.asarray(ro)[-1])
    d = _Device(e, c, ro, columns, held, source)
    for _ in range(2):
        got, msg = d.call()
        assert got == nnz and not msg, msg
        te, tc, tro, src = d.arrays()
        assert np.array_equal(tro, wro) and np.array_equal(tc[:nnz], wc) and np.all(tc[nnz:] == -7)
        if e is not None:
            assert te[:nnz].tobytes() == we.tobytes() and np.all(te[nnz:] == 7.0)
        if source:
            assert np.array_equal(src[:nnz], wsrc) and np.all(src[nnz:] == -7)
    d.dispose()
    return te, tc, tro, src


def _csr(rows, columns):
    """rows: a list of [(column, value), ...] in stored order"""
    ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    c = np.array([j for r in rows for j, _ in r], dtype=np.int32)
    e = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return e, c, ro, columns


_3x5 = [[(3, 1.5), (1, -2.0)], [], [(1, 4.0), (3, 0.5), (3, -0.25)]]            # columns 0, 2 and 4 (first, middle, last) are stored by nobody
SMALL = {
    "1x1": lambda: _csr([[(0, 3.0)]], 1),
    "1x5": lambda: _csr([[(4, 1.0), (0, 2.0), (2, 3.0), (0, 4.0)]], 5),
    "5x1": lambda: _csr([[(0, 1.0)], [], [(0, 2.0), (0, 3.0)], [], [(0, 4.0)]], 1),
    "3x5-empty-rows-and-columns": lambda: _csr(_3x5, 5),
    "5x3-empty-rows-and-columns": lambda: _csr([[], [(2, 1.5), (0, -2.0)], [], [(0, 4.0), (2, 0.5), (2, -0.25)], []], 3),
    "no-entries": lambda: _csr([[], [], [], []], 3),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_and_rectangular_matrices(name):
    _assert_transposes(*SMALL[name]())


def test_entries_beyond_the_end_of_the_offsets_are_ignored():
    e, c, ro, columns = _csr(_3x5, 5)
    _assert_transposes(np.r_[e, 9.0, 9.0, 9.0], np.r_[c, 0, 99, -4].astype(np.int32), ro, columns)       # (columns out of range among them)
    e, c, ro, columns = SMALL["no-entries"]()
    _assert_transposes(np.full(5, 9.0), np.array([0, 1, 2, 99, -1], dtype=np.int32), ro, columns)


SYSTEMS = {
    "random1037": lambda: problems.random_nonsymmetric(1037),                         # no multiple of 64 or 256
    "random1037-reversed": lambda: reversed_rows(problems.random_nonsymmetric(1037)),
    "upwind-duplicates": lambda: with_duplicates(NONSYMMETRIC["upwind12x10x8"]()),    # 0.25 v next to 0.75 v: the stored order shows
    "mgcg_main600": lambda: problems.mgcg_main(600),                                  # 159 entries a row (and a column): the LDS class
}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_systems(name):
    s = SYSTEMS[name]()
    e, c, ro = csr_of(s)
    te, tc, tro, _ = _assert_transposes(e, c, ro, s.Count)
    print(f"{name}: {s.Count} rows, {s.nnz} entries, longest column {int(np.diff(tro).max())}")
    # the Python routines are the same call
    pe, pc, pro, psrc = amg.csr_transpose_gpu(e, c, ro, s.Count, with_source=True)
    we, wc, wro, wsrc = transpose_arrays(e, c, ro, s.Count)
    assert np.array_equal(pro, wro) and np.array_equal(pc, wc) and pe.tobytes() == we.tobytes() and np.array_equal(psrc, wsrc)
    T = amg.transpose_gpu(s)
    assert np.array_equal(T.RowOffsets, wro) and np.array_equal(T.ColumnIndeces, wc) and T.Elements.tobytes() == we.tobytes()
    assert T.b.tobytes() == np.asarray(s.b, dtype=np.float64).tobytes() and T.grid == s.grid and T.name == s.name + "-T"
    assert len(amg.csr_transpose_gpu(e, c, ro, s.Count)) == 3


def test_values_are_bit_copies():
    special = np.array([-0.0, np.inf, -np.inf, 0.0, 1.0, 5e-324], dtype=np.float64)
    nans = np.array([0x7ff8000000000001, 0xfff0000000000abc], dtype=np.uint64).view(np.float64)        # two NaNs of different payload
    e = np.r_[special, nans]
    rows = [[(2, 0), (0, 1)], [(1, 2), (2, 3), (2, 4)], [(0, 5), (1, 6), (0, 7)]]
    _, c, ro, columns = _csr(rows, 3)
    te, _, _, src = _assert_transposes(e, c, ro, columns)
    assert te.view(np.uint64).tolist() == e[src].view(np.uint64).tolist() and np.signbit(te[list(src).index(0)])


@pytest.mark.parametrize("source", [False, True])
def test_pattern_only(source):
    s = SYSTEMS["random1037-reversed"]()
    _, c, ro = csr_of(s)
    _assert_transposes(None, c, ro, s.Count, source=source)


# the arrow matrix: column 0 is stored by every row, every other column once
ARROWS = {"short-max": SHORT_MAX, "short-max+1": SHORT_MAX + 1, "lds-max": LDS_MAX, "lds-max+1": LDS_MAX + 1, "global-600001": 600001}


@pytest.mark.parametrize("name", list(ARROWS))
def test_an_arrow_on_both_sides_of_every_class_boundary(name):
    n = ARROWS[name]
    e, c, ro = arrow_fast(n)
    _, _, tro, _ = _assert_transposes(e, c, ro, n)
    assert tro[1] == n


@pytest.mark.parametrize("n", [SHORT_MAX // 2 + 1, LDS_MAX // 2 + 1, 3 * LDS_MAX + 5])
def test_an_arrow_with_every_entry_of_column_0_duplicated(n):
    e, c, ro = arrow_fast(n, copies=2)
    _, _, tro, _ = _assert_transposes(e, c, ro, n)
    assert tro[1] == 2 * n - 1                                  # one entry above a class boundary, or well into the last class


def test_a_tridiagonal_matrix_of_more_rows_than_the_grid_has_lanes():
    n = 600000
    i = np.arange(n)
    c = np.stack([i - 1, i, i + 1], axis=1).ravel()[1:-1].astype(np.int32)
    e = np.stack([-1.0 - i % 3, 4.0 + i % 5, -1.0 - i % 2], axis=1).ravel()[1:-1]
    ro = np.r_[0, 3 * i + 2][: n + 1].astype(np.int32)
    ro[-1] = len(c)
    assert n > LANES and len(c) > LANES and ro[1] == 2 and ro[-1] == 3 * n - 2
    _assert_transposes(e, c, ro, n)


def test_transposing_twice_gives_a_matrix_with_ascending_unique_columns_back():
    s = SYSTEMS["random1037"]()
    e, c, ro = csr_of(s)
    te, tc, tro = amg.csr_transpose_gpu(e, c, ro, s.Count)
    be, bc, bro = amg.csr_transpose_gpu(te, tc, tro, s.Count)
    assert np.array_equal(bro, ro) and np.array_equal(bc, c) and be.tobytes() == e.tobytes()
    e, c, ro, columns = _csr([[(0, 1.0), (3, 2.0)], [], [(1, 3.0), (3, 4.0), (4, 5.0)]], 5)
    te, tc, tro = amg.csr_transpose_gpu(e, c, ro, columns)
    be, bc, bro = amg.csr_transpose_gpu(te, tc, tro, 3)
    assert np.array_equal(bro, ro) and np.array_equal(bc, c) and be.tobytes() == e.tobytes()


# --------------------------------------------------------------------------- refusals once the arrays have been read
def _refused(e, c, ro, columns, words):
    d = _Device(e, c, ro, columns)
    got, msg = d.call()
    assert got == -1 and msg.startswith("MgcgCsrTranspose: ") and all(w in msg for w in words), msg
    te, tc, tro, src = d.arrays()
    assert np.all(te == 7.0) and np.all(tc == -7) and np.all(tro == -7) and np.all(src == -7)
    d.dispose()


def test_a_column_out_of_range_is_refused_and_the_smallest_offending_row_is_named():
    s = SYSTEMS["random1037"]()
    e, c, ro = csr_of(s)
    bad = c.copy()
    bad[ro[900] + 1], bad[ro[411] + 2], bad[ro[411] + 4], bad[ro[1000]] = s.Count + 5, s.Count, s.Count + 1, -1
    _refused(e, bad, ro, s.Count, [f"row 411 stores column {s.Count}, the matrix has {s.Count} columns"])
    # in range for a wider matrix
    bad = c.copy()
    bad[ro[411] + 2] = s.Count
    _assert_transposes(e, bad, ro, s.Count + 1)


def test_a_negative_column_is_refused():
    e, c, ro, columns = _csr(_3x5, 5)
    c[3] = -2
    _refused(e, c, ro, columns, ["row 2 stores column -2, the matrix has 5 columns"])


def test_descending_offsets_are_refused():
    s = SYSTEMS["random1037"]()
    e, c, ro = csr_of(s)
    bad = ro.copy()
    bad[700], bad[300] = bad[699] - 1, bad[299] - 2
    _refused(e, c, bad, s.Count, ["row 299: the row offsets descend"])
    end = ro.copy()
    end[-1] = s.nnz + 1
    _refused(e, c, end, s.Count, [f"the row offsets end at {s.nnz + 1}, the matrix holds {s.nnz} entries"])


def test_offsets_that_do_not_start_at_0_are_refused():
    e, c, ro, columns = _csr(_3x5, 5)
    ro[0] = 1
    _refused(e, c, ro, columns, ["rowOffsets[0] is 1, must be 0"])


# --------------------------------------------------------------------------- MgcgSymmetricPart and strength 1 on long columns
@pytest.mark.parametrize("n", [SHORT_MAX + 1] + ([LDS_MAX + 1] if LDS_MAX + 1 <= 16384 else []))
def test_symmetric_part_of_an_arrow_equals_the_yardstick_bit_for_bit(n):
    e, c, ro = arrow_fast(n)
    s = problems.LinearSystem(e, c, ro, np.zeros(n), np.ones(n), f"arrow{n}")
    se, sc, sro = symmetric_part_arrays(e, c, ro)
    d = _PartDevice(s, 2 * s.nnz)
    count, msg = d.call(count_only=True)
    assert count == len(se) and not msg, msg
    for _ in range(2):
        got, msg = d.call()
        assert got == len(se) and not msg, msg
        ge, gc, gro = d.arrays(got)
        assert np.array_equal(gro, sro) and np.array_equal(gc, sc) and ge.tobytes() == se.tobytes()
    d.dispose()


def _with_a_long_column(s, stored):
    """s with small negative entries of column 0 appended to the rows that do not store it, until `stored` rows do (None: every row)."""
    e, c, ro = csr_of(s)
    n = s.Count
    has = np.zeros(n, dtype=bool)
    has[np.repeat(np.arange(n), np.diff(ro))[c == 0]] = True
    add = np.nonzero(~has)[0]
    if stored is not None:
        add = add[: stored - int(has.sum())]
    extra = np.zeros(n, dtype=np.int64)
    extra[add] = 1
    ro2 = np.r_[0, np.cumsum(np.diff(ro) + extra)]
    e2, c2 = np.empty(ro2[-1]), np.empty(ro2[-1], dtype=np.int32)
    keep = np.ones(ro2[-1], dtype=bool)
    keep[ro2[1:][add] - 1] = False                              # the appended entry is the row's last
    e2[keep], c2[keep] = e, c
    e2[~keep], c2[~keep] = -0.01 - 0.001 * (add % 7), 0
    return _raw(s, e2, c2, ro2, f"{s.name}-column0x{len(add) + int(has.sum())}")


@functools.lru_cache(maxsize=None)
def _long_column_case(stored):
    s = _with_a_long_column(problems.random_nonsymmetric(3000), stored)
    return s, HierarchySym(*csr_of(s))


@pytest.mark.parametrize("stored", [SHORT_MAX + 1, None])
def test_strength_1_on_a_matrix_with_a_long_column_equals_the_yardstick(stored):
    s, H = _long_column_case(stored)
    e, c, ro = csr_of(s)
    longest = int(np.bincount(c, minlength=s.Count).max())
    assert longest == (s.Count if stored is None else stored)
    cg = _amg(s, strength="symmetric")
    print(f"{s.name}: longest column {longest}, rows per level {rows_per_level(H)}")
    assert len(H.levels) >= 2, "the case must coarsen to test anything"
    assert _lib.lib().MgStrength(cg.mg) == 1
    _assert_equal_hierarchies(cg, _levels_of(H))
    for l, L in enumerate(H.levels[:-1]):
        assert np.array_equal(cg.level_aggregates(l), L["map"]), l
    cg.Dispose()
