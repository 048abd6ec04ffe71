"""Matrices, right-hand sides and checks shared by the tests of the k-column product (spmv_block_kernel) and of the block loops' passes.

The k-column product takes one of three paths per wavefront of 64 rows (kernels_block.hip): FAST when the 64 rows hold at most 512
entries and no row more than 8, STAGED-SLOW when the span fits but a row is longer, UNSTAGED when the span holds more than 512.
``ragged_spd`` puts all three into every 256-row tile; ``span_classes`` is that rule on the host.  No GPU is needed to import this."""
import ctypes as C
import os

import numpy as np

from conjugategradient_amd import _lib, problems

FAST, STAGED_SLOW, UNSTAGED = 0, 1, 2
SPAN, TILE, SPAN_CAP, ROW_CAP = 64, 256, 512, 8            # kBTRows = 4 * 64, kBTCap, kBNG
DBL_MAX = np.finfo(np.float64).max

# local row numbers (row mod 256) of the special rows of ragged_spd
LONE_EVERY, LONE_AT = 37, 3        # rows that hold their diagonal only: 3, 40, 77, 114, 151, 188, 225
HUB_AT = 64 + 20                   # one row of 9 .. 40 entries in the second wavefront, whose other rows stay short
LONG_AT = 128 + 30                 # one row of several hundred entries in the third wavefront, whose span exceeds 512


def span_classes(row_offsets):
    """FAST / STAGED_SLOW / UNSTAGED for every 64-row span that owns a row, by the kernel's own rule."""
    ro = np.asarray(row_offsets, dtype=np.int64)
    n = len(ro) - 1
    starts = np.arange(0, n, SPAN)
    ends = np.minimum(starts + SPAN, n)
    entries = ro[ends] - ro[starts]
    longest = np.maximum.reduceat(np.diff(ro), starts)
    return np.where(entries > SPAN_CAP, UNSTAGED, np.where(longest > ROW_CAP, STAGED_SLOW, FAST))


def _runs(counts):
    """For counts (c0, c1, ...): the owner index of every element and its position 0 .. c-1 inside its run."""
    owner = np.repeat(np.arange(len(counts)), counts)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return owner, np.arange(int(counts.sum())) - first[owner]


def ragged_spd(n, seed=0):
    """Symmetric, strictly diagonally dominant with a positive diagonal (hence SPD), built without a Python loop over the rows.

    Every full 256-row tile holds, by local row number l = row mod 256:
      wavefront 0 and 3 (l < 64, l >= 192): rows of 1 .. 8 entries only -> FAST; a band (distances 1, 2, 7, each kept with probability
          0.6) and at most one far partner from a random matching, so 1 + 6 + 1 = 8 entries at the most;
      wavefront 1: the same short rows and ONE hub row (l = 84) of 9 + (tile mod 32) entries -> STAGED_SLOW between FAST neighbours;
      wavefront 2: the full band and one long row (l = 158) of 301 .. 500 entries (fewer where the matrix is too small to have that many
          partners) -> more than 512 entries in the span, UNSTAGED;
      l = 3, 40, 77, ...: rows that hold their diagonal only.
    The partners of the hub and long rows are rows of wavefront 2 of any tile (far gathers), so no short row grows.  Rows with
    row mod 3 == 1 store their columns in descending order, rows with row mod 5 == 0 in random order, the rest ascending.
    n mod 256 = 70 leaves a last tile with one full wavefront, one of 6 rows and two that own no row.

    Entry (i, j) is -(0.1 + u) / sqrt(degree_i degree_j), u uniform in [0, 1), and the diagonal 1.5 times the row's sum plus 1 + u.  With
    entries of one size for every row, the long rows' diagonals of several hundred become a handful of eigenvalues a hundred times the
    rest; once CG has resolved those (about 13 iterations), rounding brings them back and the residual NORM of any two summation
    orders of the dots -- the oracle's serial sums against numpy's pairwise ones -- differs by a factor of two while the iterates agree
    to 1e-10.  No trace tolerance means anything on such a matrix."""
    import scipy.sparse as sp

    assert n >= 4 * TILE, n
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    l = i % TILE
    lone, hub, long_ = l % LONE_EVERY == LONE_AT, l == HUB_AT, l == LONG_AT
    special = lone | hub | long_
    third = (l >= 2 * SPAN) & (l < 3 * SPAN)
    src, dst = [], []
    for d in (1, 2, 7):                                                    # the band
        a, b = i[: n - d], i[d:]
        keep = (rng.random(n - d) < np.where(third[a] & third[b], 1.0, 0.6)) & ~special[a] & ~special[b]
        src.append(a[keep])
        dst.append(b[keep])
    perm = rng.permutation(i[~special])                                    # one far partner: a random matching, every pair kept with probability 1/2
    m = len(perm) // 2
    keep = rng.random(m) < 0.5
    src.append(perm[:m][keep])
    dst.append(perm[m: 2 * m][keep])
    pool = rng.permutation(i[third & ~special])                            # partners of the hub and long rows
    hubs, longs = i[hub], i[long_]
    for rows, counts in ((hubs, 8 + (hubs // TILE) % 32), (longs, np.minimum(300 + (37 * (longs // TILE)) % 200, int(0.9 * len(pool))))):
        owner, pos = _runs(counts)
        start = rng.integers(0, len(pool), size=len(rows))
        src.append(rows[owner])
        dst.append(pool[(start[owner] + pos) % len(pool)])                 # consecutive entries of a shuffled pool: distinct
    src, dst = np.concatenate(src), np.concatenate(dst)
    pair = np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))      # (a far partner may also be a band neighbour)
    src, dst = pair // n, pair % n
    degree = np.bincount(np.concatenate([src, dst]), minlength=n)
    v = -(0.1 + rng.random(len(src))) / np.sqrt(degree[src] * degree[dst])  # every row sums to O(1): no eigenvalue far from the rest (see below)
    S = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([src, dst]), np.concatenate([dst, src]))), shape=(n, n)).tocsr()
    S.sum_duplicates()
    off = np.asarray(abs(S).sum(axis=1)).ravel()
    A = (S + sp.diags(1.5 * off + 1.0 + rng.random(n))).tocsr()
    A.sort_indices()
    row = np.repeat(i, np.diff(A.indptr))
    key = A.indices.astype(np.float64)
    key = np.where(row % 3 == 1, -key, key)
    key = np.where(row % 5 == 0, rng.random(len(key)), key)
    order = np.lexsort((key, row))
    e, c = np.ascontiguousarray(A.data[order]), np.ascontiguousarray(A.indices[order], dtype=np.int32)
    b = np.cos(0.3 * i) * (1.0 + i % 5)
    return problems.LinearSystem(e, c, A.indptr.astype(np.int32), np.zeros(n), b, f"ragged_spd{n}")


def streaming_system(n):
    """The dominant tridiagonal of tests/test_gpu_jacobi.py (-1 off the diagonal, 2.5 + (i mod 7) on it: a margin of 0.5 or more) plus,
    symmetrically with entries of -0.01, five hub rows of 12 .. 32 far partners (STAGED_SLOW) and one aligned 64-row span whose rows take
    10 far partners each (64 * 13 = 832 entries: UNSTAGED).  No row gains more than 0.33 off the diagonal, so dominance stays strict."""
    import scipy.sparse as sp
    from tests.test_gpu_jacobi import tridiagonal

    s, _ = tridiagonal(n)
    hubs = (np.arange(1, 6) * n) // 7 + 17
    counts = 12 + 5 * np.arange(5)
    owner, pos = _runs(counts)
    src = [hubs[owner]]
    dst = [(hubs[owner] + 4099 * (pos + 1)) % n]
    first = SPAN * ((n // 2) // SPAN)
    rows = np.repeat(np.arange(first, first + SPAN), 10)
    src.append(rows)
    dst.append((rows + 100_003 + 65 * np.tile(np.arange(10), SPAN)) % n)
    src, dst = np.concatenate(src), np.concatenate(dst)
    v = np.full(len(src), -0.01)
    E = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([src, dst]), np.concatenate([dst, src]))), shape=(n, n)).tocsr()
    A = (s.to_scipy() + E).tocsr()
    A.sum_duplicates()
    return problems.LinearSystem(np.ascontiguousarray(A.data), np.ascontiguousarray(A.indices, dtype=np.int32), A.indptr.astype(np.int32),
                                 np.zeros(n), s.b, f"streaming{n}")


def strictly_dominant(s):
    """Every row: a positive diagonal larger than the sum of the other entries' sizes."""
    A = s.to_scipy()
    d = A.diagonal()
    return bool((d > 0).all() and (d > np.asarray(abs(A).sum(axis=1)).ravel() - d).all())


def columns(s, k, seed=11):
    """k columns cycling through b = 1, seeded random b, b scaled by 1e-6, b = A x* with a nonzero start x.  Column j does not depend on k."""
    from oracle import oracle as O

    rng = np.random.default_rng(seed)
    n = s.Count
    B, X = np.zeros((k, n)), np.zeros((k, n))
    for j in range(k):
        kind = j % 4
        if kind == 0:
            B[j] = 1.0 + 0.25 * (j // 4)
        elif kind == 1:
            B[j] = rng.standard_normal(n)
        elif kind == 2:
            B[j] = 1e-6 * (1.0 + 0.5 * rng.random(n))
        else:
            xs = rng.standard_normal(n)
            B[j] = O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, xs)
            X[j] = rng.standard_normal(n)
    return B, X


# --------------------------------------------------------------------------- randomised shapes (the row-tile kernel's fuzz generator)
FUZZ_SEEDS = int(os.environ.get("MGCG_FUZZ_SEEDS", "12"))     # MGCG_FUZZ_SEEDS=400 for a long soak


def fuzz_k(seed):
    """The column count of a fuzz seed: seeds 0 .. 7 hit every k = 1 .. 8."""
    return seed % 8 + 1


def random_shape(seed):
    """Sizes around the tile and block boundaries, densities that mix the fast path (rows <= 7 / 8, spans <= 512) with slow blocks, empty
    rows, unsorted columns (odd seeds: every row reversed), nnz of every residue mod 4.  Returns (system, n, mean row length, rng): the
    generator goes on to draw the vectors of the test."""
    import scipy.sparse as sp

    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([200, 256, 300, 511, 512, 1000, 4096, 5000, 33333]))
    per_row = float(rng.choice([0.5, 2.0, 5.0, 7.0, 9.0]))
    k = rng.poisson(per_row, size=n)                            # row lengths; duplicates are merged below
    rows = np.repeat(np.arange(n), k)
    M = sp.coo_matrix((rng.standard_normal(rows.size), (rows, rng.integers(0, n, size=rows.size))), shape=(n, n)).tocsr()
    if seed % 3 == 0:
        M = M + sp.eye(n, format="csr")
    M = M.tocsr()
    M.sum_duplicates()
    M.sort_indices()
    data, indices, indptr = M.data.astype(np.float64), M.indices.astype(np.int32), M.indptr.astype(np.int32)
    if seed % 2 == 1:                                           # unsorted columns: reverse every row
        for i in range(n):
            data[indptr[i]:indptr[i + 1]] = data[indptr[i]:indptr[i + 1]][::-1]
            indices[indptr[i]:indptr[i + 1]] = indices[indptr[i]:indptr[i + 1]][::-1]
    return problems.LinearSystem(data, indices, indptr, np.zeros(n), np.zeros(n), "rnd"), n, per_row, rng


# --------------------------------------------------------------------------- non-finite numbers in x
def poison(s, x, seed=0):
    """Overwrites entries of the vector x (float64 or float32, length s.Count) in place: entry 0 and the first stored column of six
    spans spread over the matrix get inf, -inf and nan in turn, three other entries the largest finite number of x's type and three
    -0.0.  Returns the mask of the CLEAN rows: those that store none of the non-finite or largest-finite columns, whose products
    therefore cannot overflow.  A masked slot of a fast path gathers column 0 (or the span's first stored column) for rows that do not
    store it; its product must be dropped, not multiplied by zero."""
    ro, c = np.asarray(s.RowOffsets, dtype=np.int64), np.asarray(s.ColumnIndeces[: s.nnz])
    n = s.Count
    rng = np.random.default_rng(seed)
    first_rows = SPAN * np.unique(np.linspace(0, (n - 1) // SPAN, 6).astype(np.int64))
    first_rows = first_rows[ro[first_rows + 1] > ro[first_rows]]
    bad = np.unique(np.concatenate([[0], c[ro[first_rows]]])) if s.nnz else np.array([0])
    x[bad] = np.array([np.inf, -np.inf, np.nan])[np.arange(len(bad)) % 3]
    others = rng.permutation(np.setdiff1d(np.arange(n), bad))[:6]
    x[others[:3]] = np.finfo(x.dtype).max
    x[others[3:]] = -0.0
    dirty = np.isin(c, np.concatenate([bad, others[:3]]))
    rows = np.repeat(np.arange(n), np.diff(ro))
    return np.bincount(rows[dirty], minlength=n) == 0


def assert_poisoned_product(got, ref, clean, exact=True):
    """got against the stored-order reference of a product with a poisoned x: at least half of all rows are clean and finite in the
    reference, those rows are finite in got, and (exact) got has the reference's values, NaN where it has NaN."""
    assert clean.mean() >= 0.5 and np.isfinite(ref[clean]).all() and np.isfinite(ref).mean() >= 0.5, (clean.mean(), np.isfinite(ref).mean())
    assert not np.isfinite(ref).all()                                   # the poison reaches the rows that store it
    assert np.isfinite(got[clean]).all(), np.nonzero(~np.isfinite(got[clean]))[0][:8]
    if exact:
        assert np.array_equal(got, ref, equal_nan=True), np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0][:8]


# --------------------------------------------------------------------------- the C ABI on a matrix that lives on the device
class DeviceBlock:
    """A CSR matrix on the device and the block entry points on it, through raw vectors: no allocation grows with the longest row."""

    def __init__(self, s):
        from tests.gpu_util import dvec, ivec

        self.s, self.n, self.nnz = s, s.Count, s.nnz
        self.e, self.c, self.ro = dvec(s.Elements[: s.nnz]), ivec(s.ColumnIndeces[: s.nnz]), ivec(s.RowOffsets)

    def dispose(self):
        for v in (self.e, self.c, self.ro):
            v.Dispose()

    def product(self, h, X):
        """CsrMVBlock into a y full of NaN; X: (k, n)."""
        from tests.gpu_util import dvec

        k, n = X.shape
        dx, dy = dvec(X.reshape(-1)), dvec(np.full(k * n, np.nan))
        _lib.lib().CsrMVBlock(h.sparse, h.descr, dy.ToRawPtr(), self.e.ToRawPtr(), self.ro.ToRawPtr(), self.c.ToRawPtr(), dx.ToRawPtr(), self.nnz, n, k)
        _lib.check("CsrMVBlock")
        Y = dy.to_numpy(k * n).reshape(k, n)
        dx.Dispose()
        dy.Dispose()
        return Y

    def solve(self, h, B, X, rule, tol, min_it, max_it, trace_capacity=None, krylov=False, garbage=None):
        """SolveBlockEx (or SolveBlockKrylov).  The trace buffer is 8 entries longer than k * capacity and starts as -1.  garbage: a
        value the work vectors Ap, p, r start from.  Returns dict(ret, message, iteration, residual, status, trace (the raw buffer), cap, x, and the
        work vectors p (de-interleaved: SolveBlockEx keeps p[i * k + j]) and r as (k, n) arrays)."""
        from tests.gpu_util import dvec

        k, n = B.shape
        cap = max(max_it, min_it) + 8 if trace_capacity is None else trace_capacity
        vx, vb = dvec(X.reshape(-1)), dvec(B.reshape(-1))
        work = [dvec(np.full(k * n, 7.0 if garbage is None else garbage)) for _ in range(3)]
        it, res, st, tr = np.full(8, -7, np.int32), np.full(8, -7.0), np.full(8, -7, np.int32), np.full(k * cap + 8, -1.0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        L = _lib.lib()
        L.MgcgClearLastError()
        fn = L.SolveBlockKrylov if krylov else L.SolveBlockEx
        ret = fn(h.blas, h.sparse, h.descr, self.e.Ptr, self.ro.Ptr, self.c.Ptr, vx.Ptr, vb.Ptr, work[0].Ptr, work[1].Ptr, work[2].Ptr,
                 self.nnz, n, k, tol, min_it, max_it, rule, it.ctypes.data_as(C.POINTER(C.c_int)) if krylov else ptr(it), ptr(res), ptr(st), ptr(tr), cap)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        out = dict(ret=ret, message=msg, iteration=int(it[0]) if krylov else it[:k].copy(), residual=res[:k].copy(), status=st[:k].copy(), trace=tr, cap=cap,
                   x=vx.to_numpy(k * n).reshape(k, n), p=work[1].to_numpy(k * n).reshape(n, k).T.copy(), r=work[2].to_numpy(k * n).reshape(k, n))
        for v in [vx, vb] + work:
            v.Dispose()
        return out
