"""Aggregation multigrid on the host side (no GPU needed): the numpy yardstick of tests/test_gpu_amg.py lives here and is checked against
scipy's P^T A P, against the partition properties the matching promises and -- with 2x2x2 box maps -- against the geometric CPU oracle;
the library exports the three entry points and refuses bad arguments before it asks for a device.  The systems that a sorted scipy matrix
cannot express -- reversed rows, duplicates, one-way entries, irregular maps -- are built here from raw arrays and checked on the CPU first.

The yardstick is the algorithm of include/MgcgGpu.h (MgSetupAggregation) in np.float64 and 32-bit unsigned integers: the matching pass
round by round, the composed maps, the Galerkin product in the contract's order (members ascending, entries in stored order, every value
added to its coarse column's accumulator from +0.0, sigma * acc), and the V-cycle in the order of operations of oracle/mg_oracle.c with a
matrix row summed serially in stored order (``row_sums``).  The HIP set-up and cycle must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums, serial_sum

U32 = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------- the yardstick: matching
def edge_key(i, j):
    """The symmetric tie-break key of the edges {i, j} (arrays), 32-bit unsigned arithmetic carried in uint64 and masked."""
    i, j = np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    h = (((lo * np.uint64(0x9E3779B1)) & U32) + ((hi * np.uint64(0x85EBCA77)) & U32)) & U32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & U32
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & U32
    h ^= h >> np.uint64(15)
    return h


def candidate_edges(e, c, ro, theta):
    """(i, j, w) of every stored entry that is a candidate edge of its row: a negative off-diagonal entry with w >= theta m_i and theta m_j."""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    c = np.asarray(c, dtype=np.int64)
    w = -e
    couples = (c != rows) & (e < 0)
    m = np.zeros(n)
    np.maximum.at(m, rows[couples], w[couples])
    candidate = couples & (w >= theta * m[rows]) & (w >= theta * m[c])
    return rows[candidate], c[candidate], w[candidate]


def matching_pass(e, c, ro, theta):
    """(map, aggregates): one matching pass, aggregates numbered by their smallest member."""
    n = len(ro) - 1
    ri, cj, wk = candidate_edges(e, c, ro, theta)
    hk = edge_key(ri, cj)
    match = np.full(n, -1, dtype=np.int64)
    while True:
        live = (match[ri] < 0) & (match[cj] < 0)
        if not live.any():
            break
        a, b, ww, hh = ri[live], cj[live], wk[live], hk[live]
        order = np.lexsort((b, hh, ww, a))                     # by row, then (w, h, j) ascending: a row's pick is its last
        a, b = a[order], b[order]
        last = np.r_[a[1:] != a[:-1], True]
        pick = np.full(n, -1, dtype=np.int64)
        pick[a[last]] = b[last]
        picked = np.nonzero(pick >= 0)[0]
        mutual = picked[pick[pick[picked]] == picked]
        if len(mutual) == 0:                                   # (an unsymmetric matrix; a symmetric one always pairs its largest edge)
            break
        match[mutual] = pick[mutual]
    ids = np.arange(n)
    root = np.where(match >= 0, np.minimum(ids, match), ids)
    number = np.cumsum(root == ids) - 1
    return number[root].astype(np.int32), int(number[-1]) + 1 if n else 0


def galerkin(e, c, ro, amap, nc, sigma):
    """sigma * P^T A P in the contract's order -> (elements, columns, offsets)."""
    n = len(ro) - 1
    amap = np.asarray(amap, dtype=np.int64)
    members = np.argsort(amap, kind="stable")                  # by aggregate, ascending fine index within one
    length = np.diff(ro)[members]
    start = np.asarray(ro[:-1], dtype=np.int64)[members]
    total = int(length.sum())
    first = np.cumsum(length) - length
    k = np.repeat(start - first, length) + np.arange(total)   # the stored entries in the contract's order
    key = np.repeat(amap[members], length) * nc + amap[np.asarray(c, dtype=np.int64)[k]]
    order = np.argsort(key, kind="stable")                     # groups by (I, J), the contract's order kept inside a group
    key, vals = key[order], e[k][order]
    head = np.r_[True, key[1:] != key[:-1]] if total else np.zeros(0, dtype=bool)
    groups = np.r_[np.nonzero(head)[0], total].astype(np.int64)
    acc = row_sums(vals, np.zeros(total, dtype=np.int64), groups, np.ones(1))     # ((0 + v0) + v1) + ...: 1.0 * v is exact
    ukey = key[head]
    elements = sigma * acc
    columns = (ukey % nc).astype(np.int32)
    offsets = np.zeros(nc + 1, dtype=np.int32)
    np.add.at(offsets, ukey // nc + 1, 1)
    assert n == len(amap)
    return elements, columns, np.cumsum(offsets).astype(np.int32)


def level_map(e, c, ro, passes, theta):
    """The composed map of `passes` matching passes (pass p > 1 on the unscaled Galerkin matrix of pass p - 1) and its pass maps."""
    amap, nc, each = None, 0, []
    for p in range(1, passes + 1):
        m, count = matching_pass(e, c, ro, theta)
        each.append(m)
        amap = m if amap is None else m[amap]
        nc = count
        if count == len(ro) - 1 or p == passes:
            break
        e, c, ro = galerkin(e, c, ro, m, count, 1.0)
    return amap, nc, each


def diagonal_inverse(e, c, ro):
    """1 / (the first stored entry of column i in row i); the row index of the first row without a usable one otherwise."""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    at = np.nonzero(np.asarray(c) == rows)[0]
    r, firsts = np.unique(rows[at], return_index=True)
    d = np.zeros(n)
    d[r] = e[at[firsts]]
    bad = np.nonzero(~((d > 0) & np.isfinite(d)))[0]
    if len(bad):
        raise ValueError(f"row {int(bad[0])}")
    return 1.0 / d


class Hierarchy:
    """levels[l] = dict(e, c, ro, dinv, map, nc); built by the library's rules (maps=None) or from the caller's maps."""

    def __init__(self, e, c, ro, levels=8, passes=3, theta=0.25, minCoarse=64, omega=0.8, nu=1, nuCoarse=4, sigma=0.5, maps=None):
        self.omega, self.nu, self.nuCoarse, self.sigma = omega, nu, nuCoarse, sigma
        self.levels = []
        e, c, ro = np.asarray(e, dtype=np.float64), np.asarray(c, dtype=np.int32), np.asarray(ro, dtype=np.int32)
        if maps is not None:
            levels = len(maps) + 1
        for l in range(levels):
            try:
                L = dict(e=e, c=c, ro=ro, dinv=diagonal_inverse(e, c, ro), map=None, nc=0)
            except ValueError as err:
                raise ValueError(f"level {l}, {err}") from None
            self.levels.append(L)
            n = len(ro) - 1
            if l + 1 >= levels:
                break
            if maps is not None:
                amap = np.asarray(maps[l], dtype=np.int32)
                nc = len(maps[l + 1]) if l + 1 < len(maps) else int(amap.max()) + 1
            else:
                if n <= minCoarse:
                    break
                amap, nc, _ = level_map(e, c, ro, passes, theta)
                if 4 * nc > 3 * n:
                    break
            L["map"], L["nc"] = amap, nc
            e, c, ro = galerkin(e, c, ro, amap, nc, sigma)

    def _smooth(self, L, b, x, sweeps, first):
        for s in range(sweeps):
            if first and s == 0:
                t = L["dinv"] * b
                x = self.omega * t
            else:
                res = b - row_sums(L["e"], L["c"], L["ro"], x)
                t = L["dinv"] * res
                step = self.omega * t
                x = x + step
        return x

    def _vcycle(self, l, b):
        L = self.levels[l]
        if l == len(self.levels) - 1:
            return self._smooth(L, b, None, self.nuCoarse, True)
        x = self._smooth(L, b, None, self.nu, True)
        r = b - row_sums(L["e"], L["c"], L["ro"], x)
        members = np.argsort(L["map"], kind="stable")
        offsets = np.r_[0, np.cumsum(np.bincount(L["map"], minlength=L["nc"]))]
        bc = row_sums(np.ones(len(members)), members, offsets, r)      # the serial sum over the members, ascending, from +0.0
        ec = self._vcycle(l + 1, bc)
        x = x + ec[L["map"]]
        return self._smooth(L, b, x, self.nu, False)

    def apply(self, r):
        return self._vcycle(0, np.asarray(r, dtype=np.float64))

    def pcg(self, b, x0=None, tol=1e-8, max_it=500, dot=None, min_it=0):
        """The shell of oracle_pcg (oracle/mg_oracle.c) under RULE_CSHARP -> dict(x, iteration, residual, status, trace).  ``dot`` forms every
        sum of the loop (default: numpy's); with ``lambda a, b: serial_sum(a * b)`` it is the reference's serial left-to-right sum of the
        rounded products, the order of the library under dot_order = 1.  ``min_it`` is the library's minIteration: no iteration below it
        ends the loop on its residual or on the cap."""
        dot = (lambda u, v: float(u @ v)) if dot is None else dot
        L = self.levels[0]
        x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=np.float64)
        r = b - row_sums(L["e"], L["c"], L["ro"], x)
        z = self.apply(r)
        p = z.copy()
        rz = dot(r, z)
        trace = []
        it = 0
        while True:
            Ap = row_sums(L["e"], L["c"], L["ro"], p)
            alpha = rz / dot(p, Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            res = math.sqrt(dot(r, r))
            trace.append(res)
            if (it >= min_it and (it > max_it or res < tol)) or not math.isfinite(res):
                break
            z = self.apply(r)
            rz_new = dot(r, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
            it += 1
        converged = min_it <= it <= max_it and res < tol
        status = _lib.OK if converged else _lib.MAXIT_EXCEEDED if it >= min_it and it > max_it else _lib.NONFINITE
        return dict(x=x, iteration=it, residual=res, status=status, trace=np.array(trace))


def serial_dot(a, b):
    """The dot product of the library under dot_order = 1: the rounded products added strictly left to right from +0.0."""
    return serial_sum(a * b)


# --------------------------------------------------------------------------- the systems of the two test files
def system_of(A, name, rng=None):
    """A LinearSystem of a scipy matrix with sorted columns; b = ones, or N(0, 1) from rng."""
    A = A.tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = np.ones(n) if rng is None else rng.standard_normal(n)
    return problems.LinearSystem(A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32), np.zeros(n), b, name)


def permuted(s, seed):
    """P A P^T of a system for a seeded permutation: the same operator in another row order."""
    perm = np.random.default_rng(seed).permutation(s.Count)
    A = s.to_scipy()[perm][:, perm]
    out = system_of(A, s.name + "-permuted")
    out.b = np.asarray(s.b)[perm].copy()
    return out


def graph_laplacian(n, seed, shift=1e-3):
    """The Laplacian of the n^3 grid graph with edge weights 10^U(0, 3), plus shift * I."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    idx = np.arange(n ** 3).reshape(n, n, n)
    a = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel(), idx[:, :, :-1].ravel()])
    b = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel(), idx[:, :, 1:].ravel()])
    w = 10.0 ** rng.uniform(0.0, 3.0, len(a))
    W = sp.coo_matrix((np.r_[w, w], (np.r_[a, b], np.r_[b, a])), shape=(n ** 3, n ** 3)).tocsr()
    return system_of(sp.diags(np.asarray(W.sum(axis=1)).ravel() + shift) - W, f"graph-laplacian-{n}")


def arrowhead(n=1037, head=411, fan=320, seed=3):
    """n rows: a ring with random negative weights plus one arrowhead row (`head`) coupled to `fan` rows; strictly diagonally dominant."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    i = np.arange(n)
    a, b = i, (i + 1) % n
    w = rng.uniform(0.5, 2.0, n)
    others = rng.choice(np.delete(i, [head - 1, head, head + 1]), fan, replace=False)
    a, b, w = np.r_[a, np.full(fan, head)], np.r_[b, others], np.r_[w, rng.uniform(0.1, 3.0, fan)]
    W = sp.coo_matrix((np.r_[w, w], (np.r_[a, b], np.r_[b, a])), shape=(n, n)).tocsr()
    return system_of(sp.diags(1.25 * np.asarray(W.sum(axis=1)).ravel()) - W, "arrowhead")


def box_maps(grid, levels):
    """The 2x2x2 (2x2 in 2-D) maps of the geometric hierarchy, as far as the oracle coarsens: a list of levels - 1 maps at most."""
    nx, ny, nz = grid
    maps = []
    for _ in range(levels - 1):
        if (nx > 1 and nx % 2) or (ny > 1 and ny % 2) or (nz > 1 and nz % 2) or (nx == ny == nz == 1):
            break
        cx, cy, cz = (2 if nx > 1 else 1), (2 if ny > 1 else 1), (2 if nz > 1 else 1)
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        maps.append((((z // cz) * (ny // cy) + y // cy) * (nx // cx) + x // cx).ravel().astype(np.int32))
        nx, ny, nz = nx // cx, ny // cy, nz // cz
    return maps


def csr_of(s):
    return np.asarray(s.Elements[: s.nnz], dtype=np.float64), np.asarray(s.ColumnIndeces[: s.nnz]), np.asarray(s.RowOffsets)


# --------------------------------------------------------------------------- systems that system_of cannot make: built from raw arrays
def _raw(s, e, c, ro, name):
    """A LinearSystem of raw CSR arrays in exactly this stored order, with s's right-hand side."""
    n = len(ro) - 1
    return problems.LinearSystem(np.ascontiguousarray(e, dtype=np.float64), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(ro, dtype=np.int32),
                                 np.zeros(n), np.array(s.b, dtype=np.float64), name)


def reversed_rows(s):
    """Every row's entries in reverse stored order: the diagonal moves, no row is sorted ascending."""
    e, c, ro = csr_of(s)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    order = np.lexsort((-np.arange(s.nnz), rows))
    return _raw(s, e[order], c[order], ro, s.name + "-reversed")


def diagonal_first(s):
    """Every row with its diagonal first and the other entries by ascending column behind it."""
    e, c, ro = csr_of(s)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    order = np.lexsort((c, c != rows, rows))
    return _raw(s, e[order], c[order], ro, s.name + "-diagonal-first")


def with_duplicates(s):
    """Every off-diagonal entry v stored as the two adjacent entries 0.25 v and 0.75 v, and an explicit 0.0 of the row's own column behind
    the (one) diagonal entry: the diagonal stays the FIRST stored entry of column i."""
    e, c, ro = csr_of(s)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    diagonal = c == rows
    assert np.array_equal(np.bincount(rows[diagonal], minlength=s.Count), np.ones(s.Count, dtype=np.int64))
    e2 = np.stack([np.where(diagonal, e, 0.25 * e), np.where(diagonal, 0.0, 0.75 * e)], axis=1).ravel()
    return _raw(s, e2, np.repeat(c, 2), 2 * ro.astype(np.int64), s.name + "-duplicates")


def one_way(s, rows=150, weight=-2000.0, seed=2):
    """A symmetric M-matrix plus `rows` entries (i, (i + 37) mod n) of value `weight` that have no mirror entry, each stored at the end of its
    row, the row's diagonal raised by |weight|: every row stays diagonally dominant, the matrix is no longer symmetric."""
    e, c, ro = csr_of(s)
    n = s.Count
    where = np.sort(np.random.default_rng(seed).choice(n, rows, replace=False))
    row_of = np.repeat(np.arange(n), np.diff(ro))
    e = e.copy()
    at = np.nonzero((c == row_of) & np.isin(row_of, where))[0]
    assert len(at) == rows
    e[at] += abs(weight)
    end = np.asarray(ro, dtype=np.int64)[where + 1]           # insert behind the last entry of each chosen row
    e2, c2 = np.insert(e, end, weight), np.insert(c, end, (where + 37) % n)
    extra = np.zeros(n, dtype=np.int64)
    extra[where] = 1
    return _raw(s, e2, c2, np.r_[0, np.cumsum(np.diff(ro) + extra)], s.name + "-one-way")


def dominant_graph(n, seed):
    """The weights of graph_laplacian with the diagonal of arrowhead: 1.25 x the off-diagonal row sum, a strictly dominant M-matrix."""
    import scipy.sparse as sp

    L = graph_laplacian(n, seed, shift=0.0).to_scipy()
    W = sp.diags(L.diagonal()) - L
    return system_of(sp.diags(1.25 * np.asarray(W.sum(axis=1)).ravel()) - W, f"dominant-graph-{n}")


def path_graph(n, seed, decades=0.0):
    """A path of n rows (tridiagonal) with edge weights U(0.5, 2) (times 10^U(0, decades)) and the diagonal 1.25 x the off-diagonal row sum,
    columns ascending.  With decades = 0 every edge passes the strength threshold 0.25; with 2 the threshold decides."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, n - 1)
    if decades:
        w = w * 10.0 ** rng.uniform(0.0, decades, n - 1)
    left, right = np.r_[0.0, w], np.r_[w, 0.0]
    e = np.stack([-left, 1.25 * (left + right), -right], axis=1).ravel()
    i = np.arange(n)
    c = np.stack([i - 1, i, i + 1], axis=1).ravel()
    keep = (c >= 0) & (c < n)
    ro = np.r_[0, np.cumsum(keep.reshape(n, 3).sum(axis=1))]
    s = problems.LinearSystem(e[keep], c[keep].astype(np.int32), ro.astype(np.int32), np.zeros(n), np.ones(n), f"path-{n}")
    return s


def irregular_maps(n, seed=11):
    """Three maps no grid would give.  Level 0: aggregates of sizes drawn from 1 .. 40, their ids a random permutation (not numbered by
    first member), their members scattered over the rows by another; level 1: permutation % 5; level 2: one aggregate of everything."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 41)), n - sum(sizes)))
    ids = rng.permutation(len(sizes))
    m0 = np.empty(n, dtype=np.int32)
    m0[rng.permutation(n)] = np.repeat(ids, sizes)
    m1 = (rng.permutation(len(sizes)) % 5).astype(np.int32)
    assert len(sizes) >= 5
    return [m0, m1, np.zeros(5, dtype=np.int32)]


def pairs_with_a_negative_coarse_diagonal(blocks=100):
    """`blocks` diagonal blocks [[1, -2], [-2, 1]]: level 0 is fine, every pair is matched, the coarse diagonal sigma (1 - 2 - 2 + 1) < 0."""
    n = 2 * blocks
    i = np.arange(n)
    e = np.where(i % 2 == 0, [[1.0], [-2.0]], [[-2.0], [1.0]]).T.ravel()
    c = np.stack([i - i % 2, i - i % 2 + 1], axis=1).ravel()
    return problems.LinearSystem(e, c.astype(np.int32), (2 * np.arange(n + 1)).astype(np.int32), np.zeros(n), np.ones(n), "negative-pairs")


def zero_before_the_diagonal(s, row):
    """s with an explicit 0.0 of column `row` stored at the head of that row: the first stored entry of the column, hence the diagonal."""
    e, c, ro = csr_of(s)
    at = int(ro[row])
    extra = np.zeros(s.Count, dtype=np.int64)
    extra[row] = 1
    return _raw(s, np.insert(e, at, 0.0), np.insert(c, at, row), np.r_[0, np.cumsum(np.diff(ro) + extra)], s.name + "-zero-first")


def rows_per_level(H):
    return [len(L["ro"]) - 1 for L in H.levels]


# --------------------------------------------------------------------------- the yardstick against independent statements
def _ptap(s, amap, nc, sigma):
    import scipy.sparse as sp

    n = s.Count
    P = sp.csr_matrix((np.ones(n), (np.arange(n), amap)), shape=(n, nc))
    # from copies: csr_matrix.sum_duplicates() works in place on arrays it shares and would rewrite the system's own offsets
    A = sp.csr_matrix((np.array(s.Elements[: s.nnz]), np.array(s.ColumnIndeces[: s.nnz]), np.array(s.RowOffsets)), shape=(n, n))
    A.sum_duplicates()
    C_ = (P.T @ A @ P).tocsr() * sigma
    C_.sort_indices()
    return C_


@pytest.mark.parametrize("name", ["poisson", "poisson-permuted", "random_spd", "graph", "arrowhead"])
def test_galerkin_equals_scipy_ptap(name):
    s = {"poisson": lambda: problems.poisson(6, 5, 4), "poisson-permuted": lambda: permuted(problems.poisson(8, 6, 5), 1),
         "random_spd": lambda: problems.random_spd(700), "graph": lambda: graph_laplacian(6, 2), "arrowhead": arrowhead}[name]()
    e, c, ro = csr_of(s)
    for passes in (1, 2, 3):
        amap, nc, _ = level_map(e, c, ro, passes, 0.25)
        for sigma in (1.0, 0.5):
            ge, gc, gro = galerkin(e, c, ro, amap, nc, sigma)
            ref = _ptap(s, amap, nc, sigma)
            # scipy drops nothing here: an entry that cancels to 0.0 stays stored in both
            assert np.array_equal(gro, ref.indptr) and np.array_equal(gc, ref.indices), (name, passes)
            if name.startswith("poisson"):
                assert np.array_equal(ge, ref.data)            # integer values: every order of summation gives the same bits
            else:
                assert np.abs(ge - ref.data).max() <= 1e-13 * np.abs(ref.data).max()


@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_every_map_is_a_partition_into_small_aggregates(passes):
    for s in (permuted(problems.poisson(9, 7, 5), 4), problems.random_spd(900), graph_laplacian(7, 5), arrowhead()):
        e, c, ro = csr_of(s)
        amap, nc, each = level_map(e, c, ro, passes, 0.25)
        assert len(amap) == s.Count and amap.min() == 0 and amap.max() == nc - 1
        sizes = np.bincount(amap, minlength=nc)
        assert sizes.min() >= 1 and sizes.max() <= 2 ** passes
        assert all(np.bincount(m).max() <= 2 for m in each)                       # a pass pairs
        firsts = np.full(nc, s.Count)
        np.minimum.at(firsts, amap, np.arange(s.Count))
        assert np.all(np.diff(firsts) > 0)                                        # numbered by the smallest member, ascending
        # a pair is a candidate edge of the first pass's matrix: both ends hold a negative entry for the other
        A = s.to_scipy()
        m0 = each[0]
        members = np.argsort(m0, kind="stable")
        pairs = members[np.repeat(np.bincount(m0) == 2, np.bincount(m0))].reshape(-1, 2)
        assert np.all(np.asarray(A[pairs[:, 0], pairs[:, 1]]).ravel() < 0)


def test_matching_takes_the_heaviest_edge_and_needs_negative_couplings():
    import scipy.sparse as sp

    # a path 0 - 1 - 2 - 3 with weights 1, 5, 1: the middle edge is matched, the ends stay single (their edge is weaker than theta * 5)
    W = sp.diags([[1.0, 5.0, 1.0], [1.0, 5.0, 1.0]], [1, -1])
    s = system_of(sp.diags([2.0, 7.0, 7.0, 2.0]) - W, "path")
    amap, nc = matching_pass(*csr_of(s), 0.25)
    assert amap.tolist() == [0, 1, 1, 2] and nc == 3
    # positive off-diagonal entries do not couple: every row stays alone
    s = system_of(sp.diags([2.0, 7.0, 7.0, 2.0]) + W, "positive")
    amap, nc = matching_pass(*csr_of(s), 0.25)
    assert amap.tolist() == [0, 1, 2, 3] and nc == 4
    H = Hierarchy(*csr_of(s), minCoarse=1)
    assert len(H.levels) == 1


def test_edge_key_is_symmetric_and_32_bit():
    i, j = np.array([0, 5, 70000, 2 ** 31 - 2]), np.array([1, 3, 12, 2 ** 31 - 1])
    h = edge_key(i, j)
    assert np.array_equal(h, edge_key(j, i)) and h.max() <= 0xFFFFFFFF
    lo, hi = 3, 5                                               # one key by hand, Python integers
    k = (lo * 0x9E3779B1 + hi * 0x85EBCA77) & 0xFFFFFFFF
    k ^= k >> 15
    k = (k * 0x2C1B3C6D) & 0xFFFFFFFF
    k ^= k >> 12
    k = (k * 0x297A2D39) & 0xFFFFFFFF
    k ^= k >> 15
    assert int(h[1]) == k


def test_box_maps_reproduce_the_geometric_oracle(oracle):
    s = problems.poisson(8, 12, 4)
    r = np.random.default_rng(5).standard_normal(s.Count)
    for levels, nu, nuc in ((3, 1, 4), (2, 2, 3), (1, 1, 5), (3, 3, 1)):
        M = oracle.Multigrid(s, levels=levels, nu=nu, nu_coarse=nuc)
        maps = box_maps(s.grid, levels)
        H = Hierarchy(*csr_of(s), omega=M.omega, nu=nu, nuCoarse=nuc, sigma=0.5, maps=maps)
        assert len(H.levels) == M.levels
        for l, L in enumerate(H.levels):
            eo, co, ro = M.level_csr(l)
            assert np.array_equal(L["ro"], ro) and np.array_equal(L["c"], co) and np.array_equal(L["e"], eo)
            assert np.array_equal(L["dinv"], M.level_dinv(l))
        assert np.array_equal(H.apply(r), M.apply(r)), (levels, nu, nuc)


def test_yardstick_cycle_is_symmetric_and_cuts_iterations():
    s = permuted(problems.poisson(12, 12, 12), 7)
    H = Hierarchy(*csr_of(s), levels=3, omega=6.0 / 7.0)
    assert len(H.levels) == 3
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal(s.Count), rng.standard_normal(s.Count)
    a, b = float(u @ H.apply(v)), float(v @ H.apply(u))
    assert abs(a - b) <= 1e-12 * abs(a)
    out = H.pcg(np.asarray(s.b))
    A = s.to_scipy()
    assert np.linalg.norm(s.b - A @ out["x"]) < 2e-8 and out["iteration"] < 30
    with pytest.raises(ValueError, match="row 0"):
        diagonal_inverse(np.array([1.0, 2.0]), np.array([1, 1]), np.array([0, 1, 2]))


# --------------------------------------------------------------------------- the serial-dot loop and the raw-array systems
@pytest.mark.parametrize("dims", [(8, 12, 4), (16, 16, 16)])
def test_serial_dot_pcg_equals_the_geometric_oracle_bit_for_bit(oracle, dims):
    """The yardstick loop of the GPU solve tests, validated first: with box maps and serial dots it IS oracle_pcg."""
    s = problems.poisson(*dims)
    s.b[:] = np.random.default_rng(3).standard_normal(s.Count)
    M = oracle.Multigrid(s, levels=3)
    H = Hierarchy(*csr_of(s), omega=M.omega, maps=box_maps(s.grid, 3))
    assert len(H.levels) == M.levels == 3
    for min_it, max_it in ((0, 400), (25, 400), (0, 5)):
        ref = M.pcg(rule=oracle.RULE_CSHARP, min_iteration=min_it, max_iteration=max_it, trace=True)
        out = H.pcg(np.asarray(s.b), max_it=max_it, dot=serial_dot, min_it=min_it)
        assert (out["iteration"], out["status"]) == (ref["iteration"], ref["status"]), (min_it, max_it)
        assert out["trace"].tobytes() == ref["trace"].tobytes() and out["x"].tobytes() == ref["x"].tobytes()
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 6
    # the default dot is today's loop: another order of summation, the same iteration count
    assert H.pcg(np.asarray(s.b))["iteration"] == M.pcg(rule=oracle.RULE_CSHARP, trace=True)["iteration"]


BUILT = {
    "reversed": lambda: reversed_rows(permuted(problems.poisson(10, 10, 10), 7)),
    "diagonal-first": lambda: diagonal_first(permuted(problems.poisson(10, 10, 10), 7)),
    "duplicates": lambda: with_duplicates(graph_laplacian(8, 3)),
    "one-way": lambda: one_way(graph_laplacian(10, 3)),
    "dominant-graph": lambda: dominant_graph(10, 3),
    "path": lambda: path_graph(1077, 5),
    "path-wide": lambda: path_graph(1077, 5, decades=2.0),
}


@pytest.mark.parametrize("name", list(BUILT))
def test_galerkin_of_the_built_systems_equals_scipy_ptap(name):
    s = BUILT[name]()
    e, c, ro = csr_of(s)
    offsets = np.array(ro)
    for passes in (1, 3):
        amap, nc, _ = level_map(e, c, ro, passes, 0.25)
        cases = [(amap, nc)] + ([(irregular_maps(s.Count)[0], len(irregular_maps(s.Count)[1]))] if passes == 1 else [])
        for m, count in cases:
            ge, gc, gro = galerkin(e, c, ro, m, count, 0.5)
            ref = _ptap(s, m, count, 0.5)
            assert np.array_equal(gro, ref.indptr) and np.array_equal(gc, ref.indices), (name, passes)
            assert np.abs(ge - ref.data).max() <= 1e-13 * np.abs(ref.data).max()
    assert np.array_equal(s.RowOffsets, offsets)               # (the comparison left the system alone)


def test_reversed_rows_give_the_maps_of_the_sorted_matrix():
    s = permuted(problems.poisson(10, 10, 10), 7)
    H = Hierarchy(*csr_of(s), levels=3)
    assert len(H.levels) == 3
    for other in (reversed_rows(s), diagonal_first(s)):
        e, c, ro = csr_of(other)
        rows = np.repeat(np.arange(s.Count), np.diff(ro))
        first = ro[:-1]
        assert np.array_equal(ro, s.RowOffsets) and not np.array_equal(c, s.ColumnIndeces[: s.nnz])
        if other.name.endswith("reversed"):
            assert np.any(c[first] != np.arange(s.Count)) and np.all(np.diff(c)[np.diff(rows) == 0] < 0)
        else:
            assert np.all(c[first] == np.arange(s.Count))
        assert (other.to_scipy() != s.to_scipy()).nnz == 0
        G = Hierarchy(e, c, ro, levels=3)
        print(other.name, rows_per_level(G))
        assert rows_per_level(G) == rows_per_level(H)
        for L, K in zip(G.levels, H.levels):
            assert (L["map"] is None and K["map"] is None) or np.array_equal(L["map"], K["map"])
            # integer values: the order of summation cannot change a bit, the sorted coarse rows are the same rows
            assert np.array_equal(L["ro"], K["ro"]) and np.array_equal(L["dinv"], K["dinv"])


def test_duplicate_entries_coarsen_and_keep_the_first_diagonal():
    base = graph_laplacian(8, 3)
    s = with_duplicates(base)
    assert s.nnz == 2 * base.nnz
    e, c, ro = csr_of(s)
    assert np.array_equal(diagonal_inverse(e, c, ro), diagonal_inverse(*csr_of(base)))        # the 0.0 behind it is not the diagonal
    assert np.abs(s.to_scipy() - base.to_scipy()).max() <= 2.0 ** -52 * np.abs(base.Elements).max()
    H = Hierarchy(e, c, ro)
    print("duplicates", rows_per_level(H))
    assert len(H.levels) >= 3
    # a level matrix is duplicate-free whatever went in
    for L in H.levels[1:]:
        rows = np.repeat(np.arange(len(L["ro"]) - 1), np.diff(L["ro"]))
        assert np.all((np.diff(L["c"]) > 0) | (np.diff(rows) > 0))


def test_one_way_entries_end_a_pass_by_the_round_that_pairs_nobody():
    base = graph_laplacian(10, 3)
    s = one_way(base)
    assert s.nnz == base.nnz + 150
    A = s.to_scipy()
    assert (A != A.T).nnz == 300 and np.all(A @ np.ones(s.Count) > 0) and A.diagonal().min() > 0     # unsymmetric, rows dominant
    e, c, ro = csr_of(s)
    m, nc = matching_pass(e, c, ro, 0.25)
    m_sym, nc_sym = matching_pass(*csr_of(base), 0.25)
    H = Hierarchy(e, c, ro)
    print("one-way", rows_per_level(H), "aggregates of pass 1:", nc, "symmetric:", nc_sym)
    assert len(H.levels) >= 2
    assert nc != nc_sym and not np.array_equal(m, m_sym)
    # candidate edges still live between singletons: rows went on picking, so only the "nobody paired" exit can have ended the pass
    i, j, _ = candidate_edges(e, c, ro, 0.25)
    single = np.bincount(m, minlength=nc)[m] == 1
    live = int((single[i] & single[j]).sum())
    print("live candidate edges at the end of the pass:", live)
    assert live > 0
    i, j, _ = candidate_edges(*csr_of(base), 0.25)
    single = np.bincount(m_sym, minlength=nc_sym)[m_sym] == 1
    assert int((single[i] & single[j]).sum()) == 0               # the symmetric matrix ends with nothing left to pick


def test_irregular_maps_build_a_hierarchy_with_long_coarse_rows():
    s = dominant_graph(10, 3)
    maps = irregular_maps(s.Count)
    sizes = np.bincount(maps[0])
    firsts = np.full(len(sizes), s.Count)
    np.minimum.at(firsts, maps[0], np.arange(s.Count))
    assert sizes.min() >= 1 and sizes.max() > 16 and len(set(sizes)) > 5 and np.any(np.diff(firsts) < 0)
    H = Hierarchy(*csr_of(s), maps=maps)
    print("irregular", rows_per_level(H), "entries per row on level 1:", len(H.levels[1]["e"]) / len(sizes))
    assert rows_per_level(H) == [s.Count, len(sizes), 5, 1]
    assert len(H.levels[1]["e"]) > 20 * len(sizes)               # the library sums such rows by several lanes in the default mode
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal(s.Count), rng.standard_normal(s.Count)
    a, b = float(u @ H.apply(v)), float(v @ H.apply(u))
    assert abs(a - b) <= 1e-12 * abs(a)
    out = H.pcg(np.asarray(s.b))
    print("iterations", out["iteration"])
    assert out["status"] == _lib.OK and out["iteration"] < 60 and np.linalg.norm(s.b - s.to_scipy() @ out["x"]) < 2e-8
    # the identity map with sigma = 1: level 1 is the matrix itself, bit for bit
    e, c, ro = csr_of(s)
    I = Hierarchy(e, c, ro, sigma=1.0, maps=[np.arange(s.Count)])
    L = I.levels[1]
    assert np.array_equal(L["ro"], ro) and np.array_equal(L["c"], c) and L["e"].tobytes() == e.tobytes()


def test_the_yardstick_refuses_what_the_header_refuses():
    s = problems.poisson(6, 5, 4)
    with pytest.raises(ValueError, match="^row 17$"):
        diagonal_inverse(*csr_of(zero_before_the_diagonal(s, 17)))
    with pytest.raises(ValueError, match="^level 0, row 17$"):
        Hierarchy(*csr_of(zero_before_the_diagonal(s, 17)))
    p = pairs_with_a_negative_coarse_diagonal()
    e, c, ro = csr_of(p)
    m, nc = matching_pass(e, c, ro, 0.25)
    assert np.array_equal(m, np.arange(200) // 2) and nc == 100
    assert np.all(galerkin(e, c, ro, m, nc, 0.5)[0] == -1.0)
    with pytest.raises(ValueError, match="^level 1, row 0$"):
        Hierarchy(e, c, ro)
    with pytest.raises(ValueError, match="^level 1, row 0$"):
        Hierarchy(e, c, ro, maps=[m])


@pytest.mark.parametrize("n,rows", [(1, [1]), (2, [2, 1]), (3, [3, 1]), (5, [5, 1])])
def test_tiny_matrices_coarsen_to_one_row(n, rows):
    s = problems.poisson(n, 1, 1)
    H = Hierarchy(*csr_of(s), minCoarse=0)
    assert rows_per_level(H) == rows
    out = H.pcg(np.asarray(s.b))
    assert out["status"] == _lib.OK and np.linalg.norm(s.b - s.to_scipy() @ out["x"]) < 2e-8


# --------------------------------------------------------------------------- the library without a device
def test_exports_and_python_surface(hiplib):
    for name in ("MgSetupAggregation", "MgSetupAggregates", "MgLevelCopyAggregates"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3
    import conjugategradient_amd
    from conjugategradient_amd import amg, multigrid

    assert "amg" in conjugategradient_amd.__all__
    assert issubclass(amg.ConjugateGradientAmgGpu, multigrid.ConjugateGradientMgGpu)
    for member in ("level_aggregates", "Apply", "Solve", "level_csr", "level_dinv"):
        assert callable(getattr(amg.ConjugateGradientAmgGpu, member))


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    values, offsets, short = _VectorHead(None, 28, -1, b""), _VectorHead(None, 11, -1, b""), _VectorHead(None, 10, -1, b"")
    ve, vo, vs = C.addressof(values), C.addressof(offsets), C.addressof(short)
    rows = np.array([10, 4], dtype=np.int32)
    amap = np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 3], dtype=np.int32)

    def matching(blas=h, sparse=h, e=ve, r=vo, c=ve, nnz=28, count=10, levels=3, passes=3, theta=0.25):
        L.MgcgClearLastError()
        mg = L.MgSetupAggregation(blas, sparse, e, r, c, nnz, count, levels, passes, theta, 64, 0.8, 1, 4, 0.5)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return mg, msg

    def given(blas=h, sparse=h, e=ve, r=vo, c=ve, nnz=28, count=10, levels=2, level_rows=rows, maps=amap):
        L.MgcgClearLastError()
        mg = L.MgSetupAggregates(blas, sparse, e, r, c, nnz, count, levels, None if level_rows is None else level_rows.ctypes.data,
                                 None if maps is None else maps.ctypes.data, 0.8, 1, 4, 0.5)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return mg, msg

    for call, who in ((matching, "MgSetupAggregation"), (given, "MgSetupAggregates")):
        for kw in (dict(blas=None), dict(sparse=None), dict(e=None), dict(r=None), dict(c=None)):
            mg, msg = call(**kw)
            assert not mg and f"{who}: null handle" in msg, (kw, msg)
        for levels in (0, -2):
            mg, msg = call(levels=levels)
            assert not mg and f"{who}: levels {levels}, must be >= 1" in msg
        for kw in (dict(r=vs), dict(e=vs), dict(c=vs), dict(count=11), dict(nnz=29)):
            mg, msg = call(**kw)
            assert not mg and "matrix vectors too small" in msg, (kw, msg)
    for passes in (0, 5, -1):
        mg, msg = matching(passes=passes)
        assert not mg and f"passes {passes}, must be 1 .. 4" in msg
    for theta in (0.0, -0.5, 1.5, float("nan")):
        mg, msg = matching(theta=theta)
        assert not mg and "must be in (0, 1]" in msg, (theta, msg)
    # the caller's maps are read on the host: what does not fit is refused there too
    for kw, word in ((dict(level_rows=None), "null handle"), (dict(maps=None), "null handle"),
                     (dict(level_rows=np.array([9, 4], dtype=np.int32)), "levelRows[0] is 9"),
                     (dict(level_rows=np.array([10, 11], dtype=np.int32)), "levelRows[1] is 11"),
                     (dict(level_rows=np.array([10, 3], dtype=np.int32)), "row 6: aggregate id 3 out of range"),
                     (dict(level_rows=np.array([10, 5], dtype=np.int32)), "aggregate 4 is empty")):
        mg, msg = given(**kw)
        assert not mg and word in msg, (kw, msg)
    L.MgcgClearLastError()
    assert L.MgLevelCopyAggregates(None, 0, amap.ctypes.data) == -1 and "MgLevelCopyAggregates" in _lib.last_error()
    L.MgcgClearLastError()
