"""The CSR matrix product on the device (MgcgCsrMultiply) against its numpy yardstick in tests/test_multiply_host.py -- offsets, columns and
value bytes, the count-only call and two full calls of every case -- on every path of kernels_multiply.hip: the three classes of rows by
their number of products and both sides of their boundaries (and of the one-wavefront limit inside the LDS class), grid-stride loops that
take a second trip, empty rows, rows of B nobody reads, duplicates and unsorted rows in both matrices; the refusals made once the arrays
have been read; and the Python routines.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from conjugategradient_amd import _lib, amg, problems
from conjugategradient_amd.solver import ConjugateGradientGpu
from tests.gpu_util import dvec, ivec
from tests.test_amg_host import box_maps, csr_of, galerkin, reversed_rows, with_duplicates
from tests.test_amg_sym_host import NONSYMMETRIC
from tests.test_multiply_host import _csr, hand_worked, multiply_arrays, order_case, products_per_row
from tests.test_transpose_host import arrow_fast, transpose_arrays

pytestmark = pytest.mark.gpu

SHORT_MAX, LDS_MAX = amg.multiply_class_limits()
WAVE_MAX = 256                                                # inside the LDS class: rows of this many products or fewer take a one-wavefront workgroup
LANES = 2048 * 256                                            # kMaxGrid * kBlock: more rows than this and a grid-stride loop takes a second trip
PAD = 5                                                       # output entries beyond the result: they keep their fill


class _Device:
    """The CSR arrays of A and B in device vectors of the library, the two handles, and output vectors of `capacity` entries filled with
    7.0 / -7 (values None: the pattern alone)."""

    def __init__(self, a, b, columns, capacity, held=None):
        (ea, ca, roa), (eb, cb, rob) = a, b
        self.rows, self.inner, self.columns, self.capacity = len(roa) - 1, len(rob) - 1, columns, capacity
        self.heldA, self.heldB = (len(ca), len(cb)) if held is None else held
        self.blas, self.sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
        self.room = max(capacity, 1)
        self.ea, self.eb = (None, None) if ea is None else (dvec(ea), dvec(eb))
        self.roa, self.ca, self.rob, self.cb = ivec(roa), ivec(ca), ivec(rob), ivec(cb)
        self.oe = None if ea is None else dvec(np.full(self.room, 7.0))
        self.oro, self.oc = ivec(np.full(self.rows + 1, -7)), ivec(np.full(self.room, -7))

    def call(self, count_only=False):
        L = _lib.lib()
        L.MgcgClearLastError()
        ptr = lambda v: None if v is None or count_only else v.Ptr
        got = L.MgcgCsrMultiply(self.blas, self.sparse, None if self.ea is None else self.ea.Ptr, self.roa.Ptr, self.ca.Ptr, self.heldA,
                                None if self.eb is None else self.eb.Ptr, self.rob.Ptr, self.cb.Ptr, self.heldB, self.rows, self.inner, self.columns,
                                ptr(self.oe), ptr(self.oro), ptr(self.oc), 0 if count_only else self.capacity)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return got, msg

    def arrays(self):
        """(elements, columns, offsets) in their whole length (elements None where the vector was not given)"""
        return None if self.oe is None else self.oe.to_numpy(self.room), self.oc.to_numpy(self.room), self.oro.to_numpy(self.rows + 1)

    def untouched(self):
        e, c, ro = self.arrays()
        return (e is None or np.all(e == 7.0)) and np.all(c == -7) and np.all(ro == -7)

    def dispose(self):
        for v in (self.ea, self.eb, self.roa, self.ca, self.rob, self.cb, self.oe, self.oro, self.oc):
            if v is not None:
                v.Dispose()
        _lib.lib().DestroyBlas(self.blas)
        _lib.lib().DestroySparse(self.sparse)


def _same_values(got, want):
    """bit for bit; where the yardstick has a NaN, any NaN (its payload is not promised)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def _assert_multiplies(a, b, columns):
    """The count-only call and two full calls, each equal to the yardstick in every array; what lies beyond the result keeps its fill.
    a, b: (elements or None, columns, offsets).  Returns the yardstick's arrays."""
    we, wc, wro = multiply_arrays(*a, *b, columns)
    count = len(wc)
    d = _Device(a, b, columns, count + PAD)
    got, msg = d.call(count_only=True)
    assert got == count and not msg, (got, count, msg)
    assert d.untouched()
    for _ in range(2):
        got, msg = d.call()
        assert got == count and not msg, (got, count, msg)
        e, c, ro = d.arrays()
        assert np.array_equal(ro, wro) and np.array_equal(c[:count], wc) and np.all(c[count:] == -7)
        if we is not None:
            assert _same_values(e[:count], we) and np.all(e[count:] == 7.0)
    d.dispose()
    return we, wc, wro


def _pair(rows_a, inner, rows_b, columns):
    ea, ca, roa, _ = _csr(rows_a, inner)
    eb, cb, rob, _ = _csr(rows_b, columns)
    assert len(rob) - 1 == inner
    return (ea, ca, roa), (eb, cb, rob), columns


_HAND = hand_worked()
_ORDER, _ORDER_SWAPPED = order_case(), order_case(swapped=True)
SMALL = {
    "1x1.1x1": lambda: _pair([[(0, 3.0)]], 1, [[(0, -0.5)]], 1),
    "1x5.5x1": lambda: _pair([[(4, 1.0), (0, 2.0), (2, 3.0), (0, 4.0)]], 5, [[(0, 1.5)], [(0, 9.0)], [(0, -2.5)], [], [(0, 0.125), (0, 8.0)]], 1),
    "5x1.1x5": lambda: _pair([[(0, 1.0)], [], [(0, 2.0), (0, 3.0)], [], [(0, 4.0)]], 1, [[(3, 0.5), (1, -1.0), (3, 0.25)]], 5),
    "empty-rows-of-A": lambda: _pair([[], [(1, 2.0), (0, 1.0)], [], [], [(2, -1.0)], []], 3, [[(0, 1.0), (1, 2.0)], [(1, 3.0)], [(0, 4.0), (2, 5.0)]], 3),
    # rows 1 and 3 of B are pointed at by nobody; rows 0 and 4 are empty and pointed at
    "rows-of-B-nobody-reads": lambda: _pair([[(2, 1.0), (0, 5.0)], [(4, 2.0), (2, 3.0)]], 5, [[], [(0, 9.0), (1, 9.0)], [(1, 0.5), (0, 0.25)], [(2, 9.0)], []], 3),
    # columns 0, 2 and 4 (first, middle, last) of C are stored by nobody
    "columns-of-C-nobody-stores": lambda: _pair([[(0, 1.0), (1, 2.0)], [(1, 3.0)]], 2, [[(3, 1.5), (1, -2.0)], [(1, 4.0), (3, 0.5), (3, -0.25)]], 5),
    "no-entries-in-A": lambda: _pair([[], [], []], 2, [[(0, 1.0)], [(1, 2.0)]], 2),
    "no-entries-in-B": lambda: _pair([[(0, 1.0), (1, 2.0)], [(1, 3.0)]], 2, [[], []], 4),
    "no-entries-at-all": lambda: _pair([[], [], [], []], 3, [[], [], []], 2),
    "hand-worked": lambda: (_HAND[0:3], _HAND[3:6], _HAND[6]),
    "order": lambda: (_ORDER[0:3], _ORDER[3:6], _ORDER[6]),
    "order-swapped": lambda: (_ORDER_SWAPPED[0:3], _ORDER_SWAPPED[3:6], _ORDER_SWAPPED[6]),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_and_rectangular_matrices(name):
    we, wc, wro = _assert_multiplies(*SMALL[name]())
    if name == "order":
        assert we.tolist() == [0.0] and wro.tolist() == [0, 1]
    if name == "order-swapped":
        assert we.tolist() == [1.0]
    if name == "hand-worked":
        assert (we.tolist(), wc.tolist(), wro.tolist()) == ([20.0, 7.5, -7.0, 20.0], [0, 1, 0, 1], [0, 2, 2, 4])


def test_entries_beyond_the_end_of_the_offsets_are_ignored():
    (ea, ca, roa), (eb, cb, rob), columns = SMALL["hand-worked"]()
    a = (np.r_[ea, 9.0, 9.0, 9.0], np.r_[ca, 0, 99, -4].astype(np.int32), roa)              # (columns out of range among them)
    b = (np.r_[eb, 9.0, 9.0], np.r_[cb, 77, -1].astype(np.int32), rob)
    want = multiply_arrays(ea, ca, roa, eb, cb, rob, columns)
    assert [x.tolist() for x in _assert_multiplies(a, b, columns)] == [x.tolist() for x in want]
    (ea, ca, roa), (eb, cb, rob), columns = SMALL["no-entries-at-all"]()
    _assert_multiplies((np.full(4, 9.0), np.array([0, 1, 99, -1], dtype=np.int32), roa), (np.full(2, 9.0), np.array([5, -2], dtype=np.int32), rob), columns)


def test_special_values_follow_ieee():
    # row 0: a lone -0.0 product gives +0.0; row 1: inf * 0 is NaN; row 2: inf - inf is NaN; row 3: -inf stays; row 4: the smallest subnormal
    rows_a = [[(0, -0.0)], [(1, np.inf)], [(2, 1.0), (3, 1.0)], [(3, 2.0)], [(4, 1.0)]]
    rows_b = [[(0, 1.0)], [(0, 0.0)], [(1, np.inf)], [(1, -np.inf)], [(2, 5e-324)]]
    we, _, _ = _assert_multiplies(*_pair(rows_a, 5, rows_b, 3))
    assert we[0] == 0.0 and not np.signbit(we[0]) and np.isnan(we[1]) and np.isnan(we[2]) and we[3] == -np.inf and we[4] == 5e-324


# --------------------------------------------------------------------------- systems
@functools.lru_cache(maxsize=None)
def _system(name):
    s = {"random1037": lambda: problems.random_nonsymmetric(1037),                      # no multiple of 64 or 256
         "random1037-reversed": lambda: reversed_rows(problems.random_nonsymmetric(1037)),
         "upwind-duplicates": lambda: with_duplicates(NONSYMMETRIC["upwind12x10x8"]()),  # 0.25 v next to 0.75 v: the stored order shows
         "poisson12": lambda: problems.poisson(12, 12, 12),
         "mgcg_main600": lambda: problems.mgcg_main(600)}[name]()
    return s, csr_of(s)


def _transposed(m, columns):
    te, tc, tro, _ = transpose_arrays(*m, columns)
    return te, tc, tro


def _squares(name):
    s, m = _system(name)
    return m, m, s.Count


def _rectangular():
    s = problems.sparse_rectangular(900, 400)
    m = (s.Elements, s.ColumnIndeces, s.RowOffsets)
    return m, _transposed(m, 400), 900


def _first_rows_of_a_wide_matrix():
    """the first 64 rows of mgcg_main(600) times the whole matrix: some 25 000 products a row"""
    _, (e, c, ro) = _system("mgcg_main600")
    return (e[: ro[64]], c[: ro[64]], ro[:65]), (e, c, ro), 600


def _arrow_normal():
    """arrow^T arrow of 20 001 rows: row 0 has 40 001 products on 20 001 columns, every other row two products"""
    m = arrow_fast(20001)
    return _transposed(m, 20001), m, 20001


SYSTEMS = {
    "random1037-squared": lambda: _squares("random1037"),
    "random1037-reversed-squared": lambda: _squares("random1037-reversed"),
    "random1037-A.At": lambda: (_system("random1037")[1], _transposed(_system("random1037")[1], 1037), 1037),
    "random1037-At.A": lambda: (_transposed(_system("random1037")[1], 1037), _system("random1037")[1], 1037),
    "upwind-duplicates-squared": lambda: _squares("upwind-duplicates"),
    "rectangular900x400-times-its-transpose": _rectangular,
    "mgcg_main600-first-64-rows": _first_rows_of_a_wide_matrix,
    "arrow20001-normal": _arrow_normal,
}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_systems(name):
    a, b, columns = SYSTEMS[name]()
    u = products_per_row(a[1], a[2], b[2])
    _, wc, _ = _assert_multiplies(a, b, columns)
    print(f"{name}: {len(u)} rows, {int(u.sum())} products, {len(wc)} entries, most products in a row {int(u.max())}; rows in the register / LDS / "
          f"global class: {int((u <= SHORT_MAX).sum())} / {int(((u > SHORT_MAX) & (u <= LDS_MAX)).sum())} / {int((u > LDS_MAX).sum())}")
    if name == "mgcg_main600-first-64-rows":
        assert u.min() > LDS_MAX                               # the global class
    if name == "arrow20001-normal":
        assert u[0] == 40001 and np.all(u[1:] == 2)


@pytest.mark.parametrize("name", ["hand-worked", "random1037-reversed-squared"])
def test_pattern_only(name):
    a, b, columns = SMALL[name]() if name in SMALL else SYSTEMS[name]()
    _assert_multiplies((None,) + tuple(a[1:]), (None,) + tuple(b[1:]), columns)


# --------------------------------------------------------------------------- both sides of every class boundary
BOUNDARIES = {"short-max": SHORT_MAX, "short-max+1": SHORT_MAX + 1, "wave-max": WAVE_MAX, "wave-max+1": WAVE_MAX + 1, "lds-max": LDS_MAX,
              "lds-max+1": LDS_MAX + 1, "global-3-lds-max+5": 3 * LDS_MAX + 5}


def _values(rng, n):
    """10^U(-8, 8) with random signs: a sum in another order has other bits"""
    return 10.0 ** rng.uniform(-8.0, 8.0, n) * rng.choice([-1.0, 1.0], n)


def _one_entry_on_a_long_row(L, rng):
    """(a) row 1 of A has one entry, pointing at a row of B of L distinct, unsorted columns; rows 0 and 2 of A are short"""
    columns = L + 3
    long_row = list(zip((rng.permutation(L) + 2).tolist(), _values(rng, L).tolist()))
    rows_b = [[(0, 2.0)], long_row, [(columns - 1, -3.0), (0, 0.5)]]
    return _pair([[(0, 1.5), (2, 2.5)], [(1, -1.25)], [(2, 4.0)]], 3, rows_b, columns)


def _one_sum(L, rng):
    """(b) row 1 of A has L entries, each pointing at a one-entry row of B; all land on column 1: one sum of L terms"""
    ks = rng.permutation(L)
    ea = np.r_[2.0, _values(rng, L), -1.0]
    ca = np.r_[0, ks, L - 1].astype(np.int32)
    roa = np.array([0, 1, L + 1, L + 2], dtype=np.int32)
    return (ea, ca, roa), (_values(rng, L), np.ones(L, dtype=np.int32), np.arange(L + 1, dtype=np.int32)), 3


def _few_columns_with_duplicates(L, rng):
    """(c) row 0 of A has entries that repeat (duplicates in A) and point at rows of B of one entry or of one column stored twice
    (duplicates in B), and at an empty row in between; L products in all, on ceil(L / 3) columns"""
    columns, m = -(-L // 3), max(L // 2, 2)
    length = 1 + np.arange(m) % 2                              # even rows of B: one entry; odd rows: their column twice
    ks = rng.integers(0, m, L)
    total = np.cumsum(length[ks])
    cut = int(np.searchsorted(total, L))                       # the first entry at which the products reach L
    ks = ks[: cut + 1]
    if total[cut] > L:
        ks[cut] = 0                                            # (a row of one entry: exactly L)
    ks = np.insert(ks, rng.integers(0, len(ks), len(ks) // 4 + 1), m)                    # row m of B is empty
    cb = np.repeat(np.arange(m) % columns, length).astype(np.int32)
    rob = np.r_[0, np.cumsum(length), length.sum()].astype(np.int32)
    a = (_values(rng, len(ks)), ks.astype(np.int32), np.array([0, len(ks)], dtype=np.int32))
    b = (_values(rng, len(cb)), cb, rob)
    assert products_per_row(a[1], a[2], b[2]).tolist() == [L]
    return a, b, columns


@pytest.mark.parametrize("shape", ["one-entry-on-a-long-row", "one-sum", "few-columns-with-duplicates"])
@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_a_row_on_both_sides_of_every_class_boundary(name, shape):
    L = BOUNDARIES[name]
    rng = np.random.default_rng(L)
    a, b, columns = {"one-entry-on-a-long-row": _one_entry_on_a_long_row, "one-sum": _one_sum, "few-columns-with-duplicates": _few_columns_with_duplicates}[shape](L, rng)
    assert int(products_per_row(a[1], a[2], b[2]).max()) == L
    we, wc, wro = _assert_multiplies(a, b, columns)
    if shape == "one-sum":
        assert wro.tolist() == [0, 1, 2, 3] and wc.tolist() == [1, 1, 1]
    if shape == "one-entry-on-a-long-row":
        assert wro[2] - wro[1] == L


def test_a_bidiagonal_matrix_of_more_rows_than_the_grid_has_lanes_squared():
    n = 600001
    i = np.arange(n)
    c = np.stack([i - 1, i], axis=1).ravel()[1:].astype(np.int32)
    e = np.stack([-1.0 - i % 3, 4.0 + i % 5], axis=1).ravel()[1:]
    ro = np.r_[0, 2 * i + 1].astype(np.int32)
    assert n > LANES and ro[-1] == len(c) == 2 * n - 1
    m = (e, c, ro)
    assert int(products_per_row(c, ro, ro).sum()) == 4 * n - 4
    _assert_multiplies(m, m, n)


# --------------------------------------------------------------------------- refusals once the arrays have been read
def _refused(a, b, columns, message, capacity=100000):
    d = _Device(a, b, columns, capacity)
    got, msg = d.call()
    assert got == -1 and msg == "MgcgCsrMultiply: " + message, msg
    assert d.untouched()
    d.dispose()


def test_descending_offsets_are_refused_in_either_matrix():
    s, (e, c, ro) = _system("random1037")
    bad = ro.copy()
    bad[700], bad[300] = bad[699] - 1, bad[299] - 2
    _refused((e, c, bad), (e, c, ro), s.Count, "A: row 299: the row offsets descend")
    _refused((e, c, ro), (e, c, bad), s.Count, "B: row 299: the row offsets descend")
    end = ro.copy()
    end[-1] = s.nnz + 1
    _refused((e, c, ro), (e, c, end), s.Count, f"B: the row offsets end at {s.nnz + 1}, the matrix holds {s.nnz} entries")
    first = ro.copy()
    first[0] = 1
    _refused((e, c, first), (e, c, ro), s.Count, "A: rowOffsets[0] is 1, must be 0")


def test_a_column_out_of_range_is_refused_and_the_smallest_offending_row_is_named():
    s, (e, c, ro) = _system("random1037")
    bad = c.copy()
    bad[ro[900] + 1], bad[ro[411] + 2], bad[ro[411] + 4], bad[ro[1000]] = s.Count + 5, s.Count, s.Count + 1, -1
    _refused((e, bad, ro), (e, c, ro), s.Count, f"A: row 411 stores column {s.Count}, the matrix has {s.Count} columns")
    _refused((e, c, ro), (e, bad, ro), s.Count, f"B: row 411 stores column {s.Count}, the matrix has {s.Count} columns")
    bad = c.copy()
    bad[ro[5]] = -2
    _refused((e, c, ro), (e, bad, ro), s.Count, f"B: row 5 stores column -2, the matrix has {s.Count} columns")
    # in range for a wider B: columns of C up to s.Count
    bad = c.copy()
    bad[ro[411] + 2] = s.Count
    _assert_multiplies((e, c, ro), (e, bad, ro), s.Count + 1)


def test_a_capacity_below_the_count_is_refused_and_the_count_is_stated():
    s, m = _system("random1037")
    count = len(multiply_arrays(*m, *m, s.Count)[1])
    _refused(m, m, s.Count, f"outCapacity {count - 1} is below the {count} entries of the product", capacity=count - 1)
    d = _Device(m, m, s.Count, count)                          # exactly the count suffices
    got, msg = d.call()
    assert got == count and not msg, msg
    d.dispose()


# --------------------------------------------------------------------------- the Python routines
def test_the_python_routines_are_the_same_call():
    s, m = _system("poisson12")
    we, wc, wro = multiply_arrays(*m, *m, s.Count)
    e, c, ro = amg.csr_multiply_gpu(m, m, s.Count)
    assert np.array_equal(ro, wro) and np.array_equal(c, wc) and e.tobytes() == we.tobytes()
    pe, pc, pro = amg.csr_multiply_gpu((None,) + m[1:], (None,) + m[1:], s.Count)
    assert pe is None and np.array_equal(pro, wro) and np.array_equal(pc, wc)
    S = amg.multiply_gpu(s, s)
    assert np.array_equal(S.RowOffsets, wro) and np.array_equal(S.ColumnIndeces, wc) and S.Elements.tobytes() == we.tobytes()
    assert S.b.tobytes() == np.asarray(s.b, dtype=np.float64).tobytes() and S.grid == s.grid and S.name == f"{s.name}*{s.name}"
    with pytest.raises(_lib.MgcgError, match="A: row 3 stores column 1728, the matrix has 1728 columns"):
        bad = m[1].copy()
        bad[m[2][3]] = s.Count
        amg.csr_multiply_gpu((m[0], bad, m[2]), m, s.Count)


def test_the_galerkin_triple_product_equals_the_aggregation_yardstick():
    s = problems.poisson(16, 16, 16)
    e, c, ro = csr_of(s)
    amap = box_maps(s.grid, 2)[0]
    nc = int(amap.max()) + 1
    P = (np.ones(s.Count), amap.astype(np.int32), np.arange(s.Count + 1, dtype=np.int32))
    Pt = amg.csr_transpose_gpu(*P, nc)
    AP = amg.csr_multiply_gpu((e, c, ro), P, nc)
    ge, gc, gro = amg.csr_multiply_gpu(Pt, AP, nc)
    we, wc, wro = galerkin(e, c, ro, amap, nc, 1.0)
    assert np.array_equal(gro, wro) and np.array_equal(gc, wc) and ge.tobytes() == we.tobytes()
