"""Matrices and host statements of the sparse product's summation orders and of its solver epilogues, shared by
tests/test_product_cases_host.py, tests/test_gpu_products.py and tests/test_gpu_epilogues.py: the cases and their expected row sums are
built once for all of them.  No GPU is needed to import this.

The lanes-per-row kernels (spmv_vector_kernel, spmv_float_vector_kernel) have a fixed order: every product is rounded on its own, lane l
of a row's L lanes adds the products of entries l, l + L, ... in stored order from +0.0, and the L sums meet in the tree
acc_l += acc_(l + off) for off = L/2 .. 1.  ``lanes_per_row_sum`` is that order in NumPy, so the kernels can be compared bit for bit
instead of within a tolerance; ``exact_rows`` is the order-free yardstick that keeps the emulation itself honest."""
import math

import numpy as np

from conjugategradient_amd import problems

RAMP_COLS = 1024
LANES = (1, 2, 4, 8, 16, 32, 64)


def lanes_per_row_sum(elements, columns, row_offsets, x, lanes, dtype=np.float64):
    """y_i of the `lanes`-lanes-per-row kernel, in `dtype`, vectorised over the rows.  lanes = 1 is the stored-order sum."""
    assert lanes >= 1 and lanes & (lanes - 1) == 0, lanes
    ro = np.asarray(row_offsets, dtype=np.int64)
    n = len(ro) - 1
    nnz = int(ro[-1]) if n >= 0 else 0
    e = np.asarray(elements[:nnz], dtype=dtype)
    prod = e * np.asarray(x, dtype=dtype)[np.asarray(columns[:nnz], dtype=np.int64)]     # a named array: every product rounded to dtype
    assert prod.dtype == dtype
    acc = np.zeros((n, lanes), dtype=dtype)
    begin, end = ro[:-1], ro[1:]
    lane = np.arange(lanes, dtype=np.int64)
    longest = int((end - begin).max()) if n else 0
    for first in range(0, longest, lanes):                                               # one stride of every row that has one
        rows = np.nonzero(end - begin > first)[0]
        idx = begin[rows, None] + first + lane[None, :]
        live = idx < end[rows, None]
        r, l = np.nonzero(live)
        acc[rows[r], l] = acc[rows[r], l] + prod[idx[r, l]]
    off = lanes // 2
    while off > 0:
        acc[:, :off] = acc[:, :off] + acc[:, off:2 * off]
        off //= 2
    return np.ascontiguousarray(acc[:, 0])


def ramp(max_len, cols=RAMP_COLS, seed=0):
    """max_len + 1 rows by cols columns, one row of every length 0 .. max_len, the rows in shuffled order; a row's columns are drawn
    without replacement and left unsorted; values N(0,1) * 10^U(-3,3).  (Count is the number of ROWS: pass cols= to the product.)"""
    assert max_len <= cols, (max_len, cols)
    rng = np.random.default_rng(seed)
    n = max_len + 1
    length = rng.permutation(n)
    order = np.argsort(rng.random((n, cols)), axis=1)                                    # row i: a random permutation of the columns
    keep = np.arange(cols)[None, :] < length[:, None]
    c = order[keep].astype(np.int32)                                                     # (row-major: row after row, length_i of each)
    e = rng.standard_normal(c.size) * 10.0 ** rng.uniform(-3.0, 3.0, size=c.size)
    ro = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
    return problems.LinearSystem(e, c, ro, np.zeros(n), np.zeros(n), f"ramp{max_len}x{cols}")


def ramp_for(lanes):
    """The ramp of a lane count.  64 lanes: rows up to 705 entries -- two trips of the 64-lane kernel's unrolled loop (4 strides of 64 =
    256 entries a trip) and every remainder of the rolled loop behind it; the other counts: up to 12 * lanes + 1."""
    return ramp(705 if lanes == 64 else 12 * lanes + 1, RAMP_COLS, seed=lanes)


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def exact_rows(elements, columns, row_offsets, x, dtype=np.float64):
    """(exact_i, S_i): the correctly rounded sum (math.fsum) of row i's products as the kernels form them -- each rounded to `dtype` -- and
    S_i = sum_j |a_ij x_j| of the same rounded products, both as float64.

    Any order of adding those len_i numbers in `dtype` makes len_i - 1 rounding errors of at most u times a partial sum that is itself at
    most S_i (1 + u)^(len_i - 2); fsum's own rounding is at most 2^-53 S_i.  Hence
        | sum in any order - exact_i |  <=  len_i * u * S_i * (1 + len_i u)  <=  1.01 * len_i * u * S_i     for len_i u <= 0.01,
    which ``row_bound`` returns.  Rows of 0 or 1 entries have no rounding at all: bound 0 is met with equality of the values."""
    ro = np.asarray(row_offsets, dtype=np.int64)
    nnz = int(ro[-1])
    prod = (np.asarray(elements[:nnz], dtype=dtype) * np.asarray(x, dtype=dtype)[np.asarray(columns[:nnz], dtype=np.int64)]).astype(np.float64)
    n = len(ro) - 1
    exact, size = np.zeros(n), np.zeros(n)
    for i in range(n):
        p = prod[ro[i]:ro[i + 1]]
        exact[i], size[i] = math.fsum(p), math.fsum(np.abs(p))
    return exact, size


def row_bound(row_offsets, size, dtype=np.float64):
    length = np.diff(np.asarray(row_offsets, dtype=np.int64))
    assert length.max(initial=0) * unit_roundoff(dtype) <= 0.01
    return 1.01 * length * unit_roundoff(dtype) * size


def assert_rows_within_bound(got, row_offsets, exact, size, dtype=np.float64, what=""):
    """Every row of got within the any-order bound of the exact row sum; names the rows and their lengths otherwise."""
    err = np.abs(np.asarray(got, dtype=np.float64) - exact)
    bad = np.nonzero(~(err <= row_bound(row_offsets, size, dtype)))[0]
    length = np.diff(np.asarray(row_offsets, dtype=np.int64))
    assert bad.size == 0, f"{what}: {bad.size} rows beyond the any-order bound, first rows {bad[:8].tolist()} of lengths {length[bad[:8]].tolist()}"


def assert_same_rows(got, want, row_offsets, what=""):
    """np.array_equal -- a NaN equal to a NaN, to nothing else -- with the rows that differ and their lengths in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
        length = np.diff(np.asarray(row_offsets, dtype=np.int64))
        raise AssertionError(f"{what}: {bad.size} of {got.size} rows differ, first rows {bad[:8].tolist()} of lengths {length[bad[:8]].tolist()}: "
                             f"{got[bad[:4]].tolist()} != {want[bad[:4]].tolist()}")


def banded_rectangular(rows, cols):
    """A rectangular matrix of few distinct rows-as-sequences of (column - row, value), so that the lossless forms of
    MgcgSetMatrixCompression apply; every 11th row is empty, the columns of a row are not sorted.
      rows < cols ("wide"): row i holds columns i + 600, i, i + 1200;
      rows > cols ("tall"): row i < cols holds columns (i + 5) mod cols and i, the rows from `cols` on are empty.  The row-pattern
        kernel (class 3) gathers x[row] for the masked slots of an empty row, which lies beyond x for those rows: the analysis must
        not choose that form when columnCount < rowCount."""
    i = np.arange(rows)
    if rows < cols:
        assert rows + 1200 <= cols
        c = np.stack([i + 600, i, i + 1200], axis=1)
        e = np.stack([-1.0 - i % 3, 4.5 + i % 2, np.full(rows, 0.25)], axis=1)
        keep = i % 11 != 0
    else:
        c = np.stack([(i + 5) % cols, i], axis=1)
        e = np.stack([-0.5 - i % 3, 3.0 + i % 2], axis=1)
        keep = (i % 11 != 0) & (i < cols)
    ro = np.concatenate([[0], np.cumsum(keep * c.shape[1])]).astype(np.int32)
    return problems.LinearSystem(np.ascontiguousarray(e[keep].reshape(-1), dtype=np.float64), np.ascontiguousarray(c[keep].reshape(-1), dtype=np.int32), ro,
                                 np.zeros(rows), np.zeros(rows), f"banded{rows}x{cols}")


def rectangular(rows, cols, per_row, seed):
    """sp.random of the given shape and mean row length, rows left in random column order, some rows empty (every 11th row is cleared
    on top of whatever the draw leaves empty).  Count is the number of ROWS."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    M = sp.random(rows, cols, density=per_row / cols, random_state=np.random.RandomState(seed), format="coo", data_rvs=rng.standard_normal)
    keep = M.row % 11 != 0
    row, c, e = M.row[keep], M.col[keep].astype(np.int32), M.data[keep].astype(np.float64)
    order = np.lexsort((rng.random(len(e)), row))                                        # row after row, shuffled inside every row
    ro = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))]).astype(np.int32)
    s = problems.LinearSystem(np.ascontiguousarray(e[order]), np.ascontiguousarray(c[order]), ro, np.zeros(rows), np.zeros(rows), f"rect{rows}x{cols}x{per_row}")
    assert (np.diff(ro) == 0).sum() >= rows // 11 and int(c.max()) < cols
    return s


# --------------------------------------------------------------------------- kernel ids, and the cases of the GPU product tests, computed once
KERNELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)                  # MgcgSetSpmvKernel: 1 stream, 2..8 = 2^(k-2) lanes per row, 9 rows, 10 row-tile
LANE_KERNELS = (2, 3, 4, 5, 6, 7, 8)


def lanes_of(kernel):
    """Lanes per row of a listed kernel id."""
    return 2 ** (kernel - 2) if 2 <= kernel <= 8 else 1


def _ragged():
    from tests.block_cases import ragged_spd

    return ragged_spd(1350)


MATRICES = {
    "poisson": (lambda: problems.poisson(20, 17, 13), None),
    "ragged": (_ragged, None),
    "mgcg700": (lambda: problems.mgcg_main(700, 24), None),
    "rect700x1900x8": (lambda: rectangular(700, 1900, 8, 1), 1900),
    "rect700x1900x40": (lambda: rectangular(700, 1900, 40, 2), 1900),
    "rect1900x700x8": (lambda: rectangular(1900, 700, 8, 3), 700),
    "rect1900x700x40": (lambda: rectangular(1900, 700, 40, 4), 700),
    "wide-bands": (lambda: banded_rectangular(700, 1900), 1900),
    "tall-bands": (lambda: banded_rectangular(1900, 700), 700),
}
MATRICES.update({f"ramp{lanes}": ((lambda lanes=lanes: ramp_for(lanes)), RAMP_COLS) for lanes in LANES})
_cases, _sums = {}, {}


class Case:
    """A matrix of MATRICES (or any system handed in) with its vectors, every one from a seed of its own: x (columns), and by row w, y0
    and the epilogue operands b, xo, dinv (positive, 10^U(-3, 3)) and d."""

    def __init__(self, name, system=None, cols=None):
        if system is None:
            build, cols = MATRICES[name]
            system = build()
        self.name, self.s = name, system
        self.rows, self.cols = self.s.Count, self.s.Count if cols is None else cols
        seed = sum(map(ord, name))
        self.x = np.random.default_rng(seed).standard_normal(self.cols)
        self.w = np.random.default_rng(seed + 1).standard_normal(self.rows)         # another seed than x: never the same vector
        self.y0 = np.random.default_rng(seed + 2).standard_normal(self.rows)
        self.b = np.random.default_rng(seed + 3).standard_normal(self.rows)
        self.xo = np.random.default_rng(seed + 4).standard_normal(self.rows)
        self.dinv = 10.0 ** np.random.default_rng(seed + 5).uniform(-3.0, 3.0, self.rows)
        self.d = np.random.default_rng(seed + 6).standard_normal(self.rows)
        for v in (self.x, self.w, self.y0, self.b, self.xo, self.dinv, self.d):
            v.setflags(write=False)
        self.A = None

    def device(self):
        if self.A is None:
            from tests.gpu_util import DeviceCsr

            self.A = DeviceCsr(self.s)
        return self.A


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def ramp_of(kernel):
    """The ramp of a kernel id: its lane count's, and the longest one for the stored-order kernels."""
    return case(f"ramp{lanes_of(kernel)}" if kernel in (3, 4, 5, 6, 7, 8) else "ramp64")


def row_sums(c, lanes, oracle):
    """A x as a kernel of `lanes` lanes per row forms it: the oracle's product for one lane, the emulation otherwise."""
    key = (c.name, lanes)
    if key not in _sums:
        s = c.s
        _sums[key] = (oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, c.x) if lanes == 1
                      else lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, c.x, lanes))
        _sums[key].setflags(write=False)
    return _sums[key]


def analysis_class(hh):
    """MgcgAnalysisInfo's class of the first matrix analysed on the handle."""
    import ctypes as C

    from conjugategradient_amd import _lib

    d, v, r, n = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong()
    return _lib.lib().MgcgAnalysisInfo(hh.sparse, 0, C.byref(d), C.byref(v), C.byref(r), C.byref(n))


# --------------------------------------------------------------------------- the solver epilogues (include/MgcgGpu.h: MgcgCsrMVEpilogue)
EPI_RESIDUAL, EPI_JACOBI, EPI_RESIDUAL_DOT, EPI_JACOBI_DOT, EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT = 2, 3, 4, 6, 7, 8
EPILOGUES = (EPI_RESIDUAL, EPI_RESIDUAL_DOT, EPI_JACOBI, EPI_JACOBI_DOT, EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT)
EPI_NAMES = {EPI_RESIDUAL: "residual", EPI_RESIDUAL_DOT: "residual-dot", EPI_JACOBI: "jacobi", EPI_JACOBI_DOT: "jacobi-dot",
             EPI_CHEBYSHEV: "chebyshev", EPI_CHEBYSHEV_DOT: "chebyshev-dot"}
EPI_OPERATIONS = {EPI_RESIDUAL: 1, EPI_RESIDUAL_DOT: 1, EPI_JACOBI: 4, EPI_JACOBI_DOT: 4, EPI_CHEBYSHEV: 5, EPI_CHEBYSHEV_DOT: 5}   # rounded operations behind acc


def epilogue_value(epi, acc, b, xo=None, dinv=None, omega=None, d=None, c1=None, c2=None):
    """spmv_epilogue_value (csrc/kernels_spmv.hip) on float64 arrays, every product and sum a NumPy operation of its own and therefore
    rounded on its own (the library is built without contraction).  dinv: an array or one number.  Returns (y, d_new, terms): d_new is the
    Chebyshev step's new d (None otherwise), terms the rounded terms of the fused sum -- r r, or b y -- (None for an epilogue without one)."""
    acc, b = np.asarray(acc, dtype=np.float64), np.asarray(b, dtype=np.float64)
    res = b - acc
    dn = None
    if epi in (EPI_RESIDUAL, EPI_RESIDUAL_DOT):
        y = res
    elif epi in (EPI_JACOBI, EPI_JACOBI_DOT):
        t = dinv * res
        s = omega * t
        y = xo + s
    elif epi in (EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT):
        t = dinv * res
        p = c1 * d
        q = c2 * t
        dn = p + q
        y = xo + dn
    else:
        raise ValueError(epi)
    terms = y * y if epi == EPI_RESIDUAL_DOT else b * y if epi in (EPI_JACOBI_DOT, EPI_CHEBYSHEV_DOT) else None
    assert y.dtype == np.float64 and (dn is None or dn.dtype == np.float64) and (terms is None or terms.dtype == np.float64)
    return y, dn, terms
