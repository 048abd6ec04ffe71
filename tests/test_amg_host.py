"""Aggregation multigrid on the host side (no GPU needed): the numpy yardstick of tests/test_gpu_amg.py lives here and is checked against
scipy's P^T A P, against the partition properties the matching promises and -- with 2x2x2 box maps -- against the geometric CPU oracle;
the library exports the three entry points and refuses bad arguments before it asks for a device.

The yardstick is the algorithm of include/MgcgGpu.h (MgSetupAggregation) in np.float64 and 32-bit unsigned integers: the matching pass
round by round, the composed maps, the Galerkin product in the contract's order (members ascending, entries in stored order, every value
added to its coarse column's accumulator from +0.0, sigma * acc), and the V-cycle in the order of operations of oracle/mg_oracle.c with a
matrix row summed serially in stored order (``row_sums``).  The HIP set-up and cycle must EQUAL it."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_mixed_host import row_sums

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


def matching_pass(e, c, ro, theta):
    """(map, aggregates): one matching pass, aggregates numbered by their smallest member."""
    n = len(ro) - 1
    rows = np.repeat(np.arange(n), np.diff(ro))
    c = np.asarray(c, dtype=np.int64)
    w = -e
    couples = (c != rows) & (e < 0)
    m = np.zeros(n)
    np.maximum.at(m, rows[couples], w[couples])
    candidate = couples & (w >= theta * m[rows]) & (w >= theta * m[c])
    ri, cj, wk = rows[candidate], c[candidate], w[candidate]
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
            L = dict(e=e, c=c, ro=ro, dinv=diagonal_inverse(e, c, ro), map=None, nc=0)
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

    def pcg(self, b, x0=None, tol=1e-8, max_it=500):
        """The shell of oracle_pcg (oracle/mg_oracle.c) under RULE_CSHARP with min_iteration 0 -> dict(x, iteration, residual, trace)."""
        L = self.levels[0]
        x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=np.float64)
        r = b - row_sums(L["e"], L["c"], L["ro"], x)
        z = self.apply(r)
        p = z.copy()
        rz = float(r @ z)
        trace = []
        it = 0
        while True:
            Ap = row_sums(L["e"], L["c"], L["ro"], p)
            alpha = rz / float(p @ Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            res = math.sqrt(float(r @ r))
            trace.append(res)
            if it > max_it or res < tol or not math.isfinite(res):
                break
            z = self.apply(r)
            rz_new = float(r @ z)
            p = z + (rz_new / rz) * p
            rz = rz_new
            it += 1
        return dict(x=x, iteration=it, residual=res, trace=np.array(trace))


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


# --------------------------------------------------------------------------- the yardstick against independent statements
def _ptap(s, amap, nc, sigma):
    import scipy.sparse as sp

    n = s.Count
    P = sp.csr_matrix((np.ones(n), (np.arange(n), amap)), shape=(n, nc))
    C_ = (P.T @ s.to_scipy() @ P).tocsr() * sigma
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
