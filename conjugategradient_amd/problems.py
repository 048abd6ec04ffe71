"""Linear systems the reference hard-codes, plus the BASELINE.json stencil configs.

Pure numpy, host side only: these build the (A, x0, b) triples that a caller of
the reference would hand to ``Initialize()``.  The CSR arrays use the
reference's field names (``Elements``, ``ColumnIndeces``, ``RowOffsets`` --
Mgcg/cuBlas/Mgcg/SparseMatrix.cs:13-23), fp64 values and 0-based int32 indices.

The large structured configs (7-point 512^3) are generated directly in HBM by
the device generator (``MgcgGeneratePoisson`` in include/MgcgGpu.h);
``poisson()`` here is its host twin for small grids and for tests.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class LinearSystem:
    """A, x0, b with the reference's member names (LinerEquations.cs:6-47)."""

    Elements: np.ndarray        # float64[nnz]
    ColumnIndeces: np.ndarray   # int32[nnz]
    RowOffsets: np.ndarray      # int32[Count+1]
    x: np.ndarray               # float64[Count]  initial guess
    b: np.ndarray               # float64[Count]
    name: str = ""
    grid: tuple | None = None   # (nx, ny, nz) for structured problems

    @property
    def Count(self) -> int:
        return int(self.x.shape[0])

    @property
    def nnz(self) -> int:
        return int(self.RowOffsets[-1])

    def to_scipy(self):
        import scipy.sparse as sp

        return sp.csr_matrix(
            (self.Elements[: self.nnz], self.ColumnIndeces[: self.nnz], self.RowOffsets),
            shape=(self.Count, self.Count),
        )


def tridiagonal(n: int) -> LinearSystem:
    """[1 2 1] central-difference matrix of
    SimpleConjugateGradient/SimpleConjugateGradient/SimpleConjugateGradient.cu:139-197
    (and SimpleConjugateGradientCpu.cpp:40-105): each row stores diagonal, left,
    right in that order; ``b[i] = i * i * 0.5`` with ``i * i`` evaluated in
    32-bit ``int`` exactly as the C++ does (it wraps for i > 46340 at N=65536);
    x0 = 0.
    """
    i = np.arange(n, dtype=np.int64)
    has_l = i > 0
    has_r = i < n - 1
    cnt = 1 + has_l.astype(np.int64) + has_r.astype(np.int64)
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=ro[1:])
    nnz = int(ro[-1])
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float64)
    col[ro[:-1]] = i
    val[ro[:-1]] = 2.0
    col[ro[:-1][has_l] + 1] = i[has_l] - 1
    val[ro[:-1][has_l] + 1] = 1.0
    pos_r = ro[:-1] + 1 + has_l
    col[pos_r[has_r]] = i[has_r] + 1
    val[pos_r[has_r]] = 1.0
    ii = (i * i).astype(np.int32)  # int overflow as in the C++ expression
    b = ii.astype(np.float64) * 0.5
    return LinearSystem(val, col, ro.astype(np.int32), np.zeros(n), b, f"tridiagonal{n}")


def mgcg_main(count: int = 34567 * 6, max_nonzero: int = 160, x0_div: float = 100.0) -> LinearSystem:
    """The driver system of Mgcg/cuBlas/Mgcg/MgcgMain.cs:51-104.

    Row i stores the diagonal FIRST (columns are not sorted), then every
    ``j in [max(0, i-max_nonzero/2+1), min(count, i+max_nonzero/2))``, ``j != i``
    ascending, with ``a_ij = |sin(i+j)|``; the diagonal is the sum of the row's
    off-diagonals accumulated left to right.  ``b_i = 10 cos(i)``, ``x0_i = i/100``.
    ``mgcg_main(21, 6, 10.0)`` is the dense system of R/CG.R:1-24.
    """
    half = max_nonzero // 2
    i = np.arange(count, dtype=np.int64)
    val, col, ro = _sin_band(count, np.maximum(0, i - half + 1), np.minimum(count, i + half), np.zeros(count))
    b = np.cos(i.astype(np.float64)) * 10.0
    x0 = i.astype(np.float64) / x0_div
    return LinearSystem(val, col, ro, x0, b, f"mgcgmain{count}")


def _sin_band(count: int, jlo: np.ndarray, jhi: np.ndarray, diag0: np.ndarray):
    """Rows ``i`` with the diagonal FIRST, then every ``j in [jlo_i, jhi_i)``, ``j != i`` ascending, ``a_ij = |sin(i+j)|``;
    diagonal = ``diag0_i`` plus the row's off-diagonals added left to right (MgcgMain.cs:79, MgcgCL.cs:33-40)."""
    i = np.arange(count, dtype=np.int64)
    cnt = jhi - jlo  # includes the diagonal's own slot (moved to the front)
    ro = np.zeros(count + 1, dtype=np.int64)
    np.cumsum(cnt, out=ro[1:])
    nnz = int(ro[-1])
    row = np.repeat(i, cnt)
    k = np.arange(nnz, dtype=np.int64) - np.repeat(ro[:-1], cnt)  # position within row
    # position 0 -> diagonal; position q>=1 -> q-th off-diagonal in ascending j
    j = np.repeat(jlo, cnt) + (k - 1)
    j = np.where(j >= row, j + 1, j)  # skip the diagonal
    col = np.where(k == 0, row, j).astype(np.int32)
    val = np.abs(np.sin((row + col).astype(np.float64)))
    val[ro[:-1]] = 0.0
    diag = np.array(diag0, dtype=np.float64)
    for q in range(int(cnt.max()) - 1):
        sel = (cnt - 1) > q
        idx = ro[:-1][sel] + 1 + q
        diag[sel] = diag[sel] + val[idx]
    val[ro[:-1]] = diag
    return val, col, ro.astype(np.int32)


def viennacl_main(n: int = 34567 * 5, band_width: int = 160) -> LinearSystem:
    """The driver system of Mgcg/ViennaCL/MgcgCL/MgcgCL.cs:14-61: ``A[i,i] = i`` is assigned first (so the dictionary row
    starts with the diagonal), then ``j in [max(0, i-band/2), min(N-1, i+band/2)]`` INCLUSIVE, ``j != i`` ascending with
    ``a_ij = |sin(i+j)|`` added onto the diagonal; ``b_i = asin(i/N)``, ``x0 = 0``; solved to 1e-4 RELATIVE."""
    half = band_width // 2
    i = np.arange(n, dtype=np.int64)
    val, col, ro = _sin_band(n, np.maximum(0, i - half), np.minimum(n - 1, i + half) + 1, i.astype(np.float64))
    # b through libm's asin, the function the C++ twin (host/MgcgCLMain.cpp) and the reference's Math.Asin call: numpy's own vectorised
    # arcsin differs from it in the last bit for ~8 % of these arguments, which would show in every bit-for-bit comparison of x
    import math
    b = np.array([math.asin(v) for v in (i.astype(np.float64) / n)])
    return LinearSystem(val, col, ro, np.zeros(n), b, f"viennaclmain{n}")


def poisson(nx: int, ny: int, nz: int = 1) -> LinearSystem:
    """5-point (nz == 1) / 7-point Poisson, Dirichlet, lexicographic x-fastest:
    diagonal 2*dim, off-diagonals -1, columns ascending (SURVEY.md section 8,
    configs 1-4).  b = 1, x0 = 0.
    """
    n = nx * ny * nz
    assert n < 2**31
    idx = np.arange(n, dtype=np.int64)
    x = idx % nx
    y = (idx // nx) % ny
    z = idx // (nx * ny)
    diag = 6.0 if nz > 1 else 4.0
    # neighbour presence in ascending column order
    masks = [z > 0, y > 0, x > 0, np.ones(n, bool), x < nx - 1, y < ny - 1, z < nz - 1]
    offs = [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
    vals = [-1.0, -1.0, -1.0, diag, -1.0, -1.0, -1.0]
    cnt = np.zeros(n, dtype=np.int64)
    for m in masks:
        cnt += m
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=ro[1:])
    nnz = int(ro[-1])
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float64)
    pos = ro[:-1].copy()
    for m, o, v in zip(masks, offs, vals):
        p = pos[m]
        col[p] = idx[m] + o
        val[p] = v
        pos += m
    return LinearSystem(val, col, ro.astype(np.int32), np.zeros(n), np.ones(n),
                        f"poisson{nx}x{ny}x{nz}", grid=(nx, ny, nz))


def poisson_nnz(nx: int, ny: int, nz: int = 1) -> int:
    n = nx * ny * nz
    nnz = n + 2 * (nx - 1) * ny * nz + 2 * nx * (ny - 1) * nz
    if nz > 1:
        nnz += 2 * nx * ny * (nz - 1)
    return nnz


def random_spd(n: int, mean_upper: float = 14.0, seed: int = 12345, sort_columns: bool = True) -> LinearSystem:
    """Config 5 of BASELINE.json: per row k ~ Poisson(mean_upper)+1
    strictly-upper random columns, values U(-1,0); A = U + U^T; diagonal =
    1 + sum|off-diag| (strictly diagonally dominant, hence SPD); b = A.1, x0 = 0.
    """
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    k = rng.poisson(mean_upper, size=n) + 1
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    # strictly-upper columns, uniform over (row, n); the last row has none
    span = n - 1 - rows
    cols = rows + 1 + np.floor(rng.random(rows.shape[0]) * np.maximum(span, 1)).astype(np.int64)
    keep = span > 0
    rows, cols = rows[keep], np.minimum(cols[keep], n - 1)
    vals = -rng.random(rows.shape[0])
    U = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    U.sum_duplicates()
    A = (U + U.T).tocsr()
    d = 1.0 + np.asarray(abs(A).sum(axis=1)).ravel()
    A = (A + sp.diags(d)).tocsr()
    A.sort_indices()
    if not sort_columns:
        # deterministic in-row shuffle: reverse every row
        ro = A.indptr
        perm = np.concatenate([np.arange(ro[i + 1] - 1, ro[i] - 1, -1) for i in range(n)]) if n < 200000 else None
        if perm is not None:
            A = sp.csr_matrix((A.data[perm], A.indices[perm], ro), shape=(n, n))
    b = A @ np.ones(n)
    return LinearSystem(np.ascontiguousarray(A.data, dtype=np.float64),
                        np.ascontiguousarray(A.indices, dtype=np.int32),
                        np.ascontiguousarray(A.indptr, dtype=np.int32),
                        np.zeros(n), b, f"random_spd{n}")


def convection_diffusion(nx: int, ny: int, nz: int = 1, c=(0.0, 0.0, 0.0), upwind: bool = False) -> LinearSystem:
    """Nonsymmetric 5-point (nz == 1) / 7-point convection-diffusion stencil on poisson()'s grid and ordering, c = (c_x, c_y[, c_z]) the
    cell Peclet numbers.  Central differences: diagonal 2 per dimension, off-diagonals -1 - c_d towards the lower neighbour and -1 + c_d
    towards the upper one.  upwind=True (first-order upwinding, c_d >= 0): diagonal 2 + 2 c_d per dimension, off-diagonals -1 - 2 c_d and
    -1.  Columns ascending; b = A.1, x0 = 0.  c = 0 gives poisson()'s matrix."""
    n = nx * ny * nz
    assert n < 2**31
    dims = 3 if nz > 1 else 2
    c = [float(v) for v in c][:dims] + [0.0] * max(0, dims - len(c))
    cx, cy, cz = c[0], c[1], (c[2] if dims == 3 else 0.0)
    idx = np.arange(n, dtype=np.int64)
    x = idx % nx
    y = (idx // nx) % ny
    z = idx // (nx * ny)
    if upwind:
        diag = sum(2.0 + 2.0 * v for v in c)
        lower = lambda v: -1.0 - 2.0 * v
        upper = lambda v: -1.0
    else:
        diag = 2.0 * dims
        lower = lambda v: -1.0 - v
        upper = lambda v: -1.0 + v
    masks = [z > 0, y > 0, x > 0, np.ones(n, bool), x < nx - 1, y < ny - 1, z < nz - 1]
    offs = [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
    vals = [lower(cz), lower(cy), lower(cx), diag, upper(cx), upper(cy), upper(cz)]
    cnt = np.zeros(n, dtype=np.int64)
    for m in masks:
        cnt += m
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=ro[1:])
    nnz = int(ro[-1])
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float64)
    pos = ro[:-1].copy()
    for m, o, v in zip(masks, offs, vals):
        p = pos[m]
        col[p] = idx[m] + o
        val[p] = v
        pos += m
    b = np.bincount(np.repeat(idx, cnt), weights=val, minlength=n)
    return LinearSystem(val, col, ro.astype(np.int32), np.zeros(n), b,
                        f"convdiff{nx}x{ny}x{nz}{'u' if upwind else 'c'}", grid=(nx, ny, nz))


def symmetric_part(system: LinearSystem) -> LinearSystem:
    """(A + A^T) / 2 of a system's matrix, with the same b, x and grid: what a V-cycle hierarchy is built from when the one of the
    nonsymmetric matrix itself is not wanted.  The pattern is the union of A's and A^T's without the sums that come to zero, columns
    ascending; every entry is one addition and one halving, so the central convection_diffusion() stencil gives poisson()'s matrix
    exactly and the diagonal is kept."""
    A = system.to_scipy().copy()                       # (to_scipy shares the system's arrays)
    A.sum_duplicates()
    H = ((A + A.T.tocsr()) * 0.5).tocsr()
    H.sort_indices()
    return LinearSystem(np.ascontiguousarray(H.data, dtype=np.float64), np.ascontiguousarray(H.indices, dtype=np.int32),
                        np.ascontiguousarray(H.indptr, dtype=np.int32), np.array(system.x, dtype=np.float64),
                        np.array(system.b, dtype=np.float64), f"{system.name}-sym", grid=system.grid)


def random_nonsymmetric(n: int, per_row: int = 9, seed: int = 12345) -> LinearSystem:
    """A random matrix with A != A^T and an uneven diagonal: per row per_row - 1 off-diagonal draws with columns uniform over the other
    rows and values N(0,1), duplicates summed; diagonal = sum |off-diagonals| + U(0.5, 50) (strictly row dominant, hence nonsingular).
    Columns ascending; b = A.1, x0 = 0."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    k = max(int(per_row) - 1, 0)
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = rng.integers(0, max(n - 1, 1), size=rows.shape[0])
    cols = cols + (cols >= rows)                       # uniform over the columns other than the row's own
    vals = rng.standard_normal(rows.shape[0])
    keep = cols < n                                    # (n == 1: no other column)
    A = sp.coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    d = np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(0.5, 50.0, size=n)
    A = (A + sp.diags(d)).tocsr()
    A.sort_indices()
    b = A @ np.ones(n)
    return LinearSystem(np.ascontiguousarray(A.data, dtype=np.float64),
                        np.ascontiguousarray(A.indices, dtype=np.int32),
                        np.ascontiguousarray(A.indptr, dtype=np.int32),
                        np.zeros(n), b, f"random_nonsymmetric{n}")


@dataclass
class LeastSquaresSystem:
    """A (Rows x Columns, CSR) and b (Rows entries) of a least-squares problem min || A x - b ||_2 (``lsqr.LeastSquaresGpu.load``)."""

    Elements: np.ndarray        # float64[nnz]
    ColumnIndeces: np.ndarray   # int32[nnz]
    RowOffsets: np.ndarray      # int32[Rows+1]
    b: np.ndarray               # float64[Rows]
    Columns: int
    name: str = ""

    @property
    def Rows(self) -> int:
        return int(self.RowOffsets.shape[0]) - 1

    @property
    def nnz(self) -> int:
        return int(self.RowOffsets[-1])

    def to_scipy(self):
        import scipy.sparse as sp

        return sp.csr_matrix((self.Elements[: self.nnz], self.ColumnIndeces[: self.nnz], self.RowOffsets), shape=(self.Rows, self.Columns))


def least_squares(system, columns: int, b=None, name: str | None = None) -> LeastSquaresSystem:
    """The CSR arrays of anything that has ``Elements``, ``ColumnIndeces`` and ``RowOffsets`` as a rows x ``columns`` least-squares
    problem with right-hand side ``b`` (default: the system's own)."""
    ro = np.ascontiguousarray(system.RowOffsets, dtype=np.int32)
    nnz = int(ro[-1])
    rhs = np.array(system.b if b is None else b, dtype=np.float64)
    if rhs.shape[0] != ro.shape[0] - 1:
        raise ValueError(f"b holds {rhs.shape[0]} entries, the matrix has {ro.shape[0] - 1} rows")
    return LeastSquaresSystem(np.ascontiguousarray(system.Elements[:nnz], dtype=np.float64), np.ascontiguousarray(system.ColumnIndeces[:nnz], dtype=np.int32),
                              ro, rhs, int(columns), getattr(system, "name", "") if name is None else name)


def sparse_rectangular(rows: int, columns: int, per_row: int = 8, seed: int = 12345) -> LeastSquaresSystem:
    """A random sparse rows x columns matrix for least squares: every row stores min(per_row, columns) draws with columns uniform over
    [0, columns) in ascending order (a column drawn twice in a row is stored twice: the product adds both) and values N(0,1); b = N(0,1),
    in general not in the range of A.  Vectorised: 4 M x 1 M with 8 per row takes seconds."""
    rng = np.random.default_rng(seed)
    k = min(int(per_row), int(columns))
    c = np.sort(rng.integers(0, columns, size=(rows, k), dtype=np.int32), axis=1)
    e = rng.standard_normal(rows * k)
    ro = (np.arange(rows + 1, dtype=np.int64) * k).astype(np.int32)
    return LeastSquaresSystem(e, np.ascontiguousarray(c.reshape(-1)), ro, rng.standard_normal(rows), int(columns), f"sparse_rect{rows}x{columns}x{k}")


def partition_offsets(count: int, device_count: int, row_offsets=None, balance: str = "rows") -> list[int]:
    """Row-range partition of Mgcg/cuBlas/Mgcg/ConjugateGradientParallelGpu.cs:271-277:
    floor(count/device_count) rows each, the last device takes the remainder.
    balance="nnz" (not in the reference; needs row_offsets): row ranges of equal NONZERO count instead -- rank r starts at the first
    row whose offset reaches r/devices of the nonzeros.  For a matrix with uneven rows (BASELINE config 5: the last of eight
    row-count slabs holds 3.7 times the nonzeros of the first) the slowest rank sets the iteration time."""
    import math

    if balance == "nnz":
        if row_offsets is None:
            raise ValueError("balance='nnz' needs the row offsets")
        ro = np.asarray(row_offsets)
        nnz = int(ro[count]) - int(ro[0])
        targets = int(ro[0]) + (np.arange(1, device_count, dtype=np.int64) * nnz) // device_count
        cuts = np.searchsorted(ro[: count + 1], targets, side="left")
        off = [0] + [int(min(max(c, 0), count)) for c in cuts] + [count]
        for i in range(1, device_count + 1):                  # monotone (empty ranks only when there are fewer rows than ranks)
            off[i] = max(off[i], off[i - 1])
        return off
    if balance != "rows":
        raise ValueError("balance must be 'rows' or 'nnz'")
    off = [0] * (device_count + 1)
    for i in range(1, device_count):
        off[i] = off[i - 1] + int(math.floor(float(count) / device_count))
    off[device_count] = count
    return off
