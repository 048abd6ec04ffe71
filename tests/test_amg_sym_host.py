"""Aggregation multigrid that matches on the symmetric part (MgSetupAggregationEx with strength = 1, MgcgSymmetricPart) on the host side
(no GPU needed): the numpy yardstick of tests/test_gpu_amg_sym.py lives here and is checked against the dense (A + A^T) / 2, against
``problems.symmetric_part`` and on the rows a sorted scipy matrix cannot express; the capability it buys -- a nonsymmetric stencil that
coarsens -- is shown on the yardstick; the library exports the entry points and refuses bad arguments before it asks for a device.

``symmetric_part_arrays`` is the contract of include/MgcgGpu.h (MgcgSymmetricPart) in np.float64: row i stores every column j that row i
of A stores or whose row j stores i, columns ascending and once each; acc = +0.0, plus row i's stored entries of column j in stored
order, plus row j's stored entries of column i in stored order; s_ij = 0.5 * acc.  A zero sum stays stored.  ``HierarchySym`` is
``Hierarchy`` (tests/test_amg_host.py) with every level's map taken from the symmetric part of that level's own matrix; the level
matrices stay sigma * P^T A P of A itself.  The HIP routines must EQUAL both."""
import ctypes as C
import inspect
import time

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import (Hierarchy, _VectorHead, csr_of, diagonal_inverse, galerkin, level_map, reversed_rows, rows_per_level, system_of,
                                 with_duplicates)
from tests.test_bicgstab_mg_host import pbicgstab_oracle
from tests.test_mixed_host import row_sums


# --------------------------------------------------------------------------- the yardstick
def symmetric_part_arrays(e, c, ro):
    """(elements, columns, offsets) of S = (A + A^T) / 2 by the contract: one serial sum from +0.0 per stored pair, halved once."""
    e, c, ro = np.asarray(e, dtype=np.float64), np.asarray(c, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    n, nnz = len(ro) - 1, len(e)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    k = np.arange(nnz, dtype=np.int64)
    # every stored entry twice: as (i, j) of A (half 0) and as (j, i) of A^T (half 1); within a half the stored order of A (ascending k)
    key = np.r_[rows * n + c, c * n + rows]
    half = np.r_[np.zeros(nnz, dtype=np.int64), np.ones(nnz, dtype=np.int64)]
    order = np.lexsort((np.r_[k, k], half, key))
    key, vals = key[order], np.r_[e, e][order]
    total = 2 * nnz
    head = np.r_[True, key[1:] != key[:-1]] if total else np.zeros(0, dtype=bool)
    groups = np.r_[np.nonzero(head)[0], total].astype(np.int64)
    acc = row_sums(vals, np.zeros(total, dtype=np.int64), groups, np.ones(1))      # ((0 + v0) + v1) + ...: 1.0 * v is exact
    ukey = key[head]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.add.at(offsets, ukey // n + 1, 1)
    return 0.5 * acc, (ukey % n).astype(np.int32), np.cumsum(offsets).astype(np.int32)


class HierarchySym(Hierarchy):
    """Hierarchy built by the library's rules with the map of each level taken from the symmetric part of the level's own matrix."""

    def __init__(self, e, c, ro, levels=8, passes=3, theta=0.25, minCoarse=64, omega=0.8, nu=1, nuCoarse=4, sigma=0.5):
        self.omega, self.nu, self.nuCoarse, self.sigma = omega, nu, nuCoarse, sigma
        self.levels = []
        e, c, ro = np.asarray(e, dtype=np.float64), np.asarray(c, dtype=np.int32), np.asarray(ro, dtype=np.int32)
        for l in range(levels):
            try:
                L = dict(e=e, c=c, ro=ro, dinv=diagonal_inverse(e, c, ro), map=None, nc=0)
            except ValueError as err:
                raise ValueError(f"level {l}, {err}") from None
            self.levels.append(L)
            n = len(ro) - 1
            if l + 1 >= levels or n <= minCoarse:
                break
            amap, nc, _ = level_map(*symmetric_part_arrays(e, c, ro), passes, theta)
            if 4 * nc > 3 * n:
                break
            L["map"], L["nc"] = amap, nc
            e, c, ro = galerkin(e, c, ro, amap, nc, sigma)


# --------------------------------------------------------------------------- the systems of the two test files
def upwind(n, c=(2.0, 1.0, 0.5)):
    return problems.convection_diffusion(n, n, n, c, upwind=True)


def central(n, c=(0.9, 0.9, 0.9)):
    return problems.convection_diffusion(n, n, n, c)


NONSYMMETRIC = {
    "central12x10x8": lambda: problems.convection_diffusion(12, 10, 8, (0.5, 0.25, 0.0)),
    "upwind12x10x8": lambda: problems.convection_diffusion(12, 10, 8, (2.0, 1.0, 0.5), upwind=True),
    "random1500": lambda: problems.random_nonsymmetric(1500),
}


def one_way_pair():
    """n = 2, both diagonals and the single entry (0, 1): its mirror (1, 0) is not stored."""
    return problems.LinearSystem(np.array([2.0, -1.0, 3.0]), np.array([0, 1, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32),
                                 np.zeros(2), np.ones(2), "one-way-pair")


def with_a_diagonal_only_row(n=70, row=33):
    """A tridiagonal upwind-like matrix (-3, 5, -1) whose row `row` stores its diagonal alone; its neighbours still store column `row`."""
    i = np.arange(n)
    e = np.stack([np.full(n, -3.0), np.full(n, 5.0), np.full(n, -1.0)], axis=1).ravel()
    c = np.stack([i - 1, i, i + 1], axis=1).ravel()
    r = np.repeat(i, 3)
    keep = (c >= 0) & (c < n) & ((r != row) | (c == row))
    ro = np.r_[0, np.cumsum(np.bincount(r[keep], minlength=n))]
    return problems.LinearSystem(e[keep], c[keep].astype(np.int32), ro.astype(np.int32), np.zeros(n), np.ones(n), "diagonal-only-row")


def _as_scipy(e, c, ro):
    import scipy.sparse as sp

    n = len(ro) - 1
    return sp.csr_matrix((np.array(e), np.array(c), np.array(ro)), shape=(n, n))


# --------------------------------------------------------------------------- S against independent statements
@pytest.mark.parametrize("name", list(NONSYMMETRIC))
def test_symmetric_part_equals_the_dense_one_exactly_and_is_bit_symmetric(name):
    s = NONSYMMETRIC[name]()
    e, c, ro = csr_of(s)
    se, sc, sro = symmetric_part_arrays(e, c, ro)
    A = s.to_scipy().toarray()
    assert not np.array_equal(A, A.T)
    dense = (A + A.T) / 2
    S = _as_scipy(se, sc, sro)
    assert np.array_equal(S.toarray(), dense)
    # the pattern is the union of A's and A^T's, columns ascending and once each; the diagonal is A's
    rows = np.repeat(np.arange(s.Count), np.diff(sro))
    assert np.all((np.diff(sc) > 0) | (np.diff(rows) > 0))
    union = (A != 0) | (A.T != 0)
    assert len(se) == int(union.sum()) and np.all(union[rows, sc])
    assert np.array_equal(dense.diagonal(), A.diagonal())
    # bit-symmetric: the transpose, stored the same way, is the same three arrays
    T = S.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indptr, sro) and np.array_equal(T.indices, sc) and T.data.tobytes() == se.tobytes()
    if name == "random1500":                                   # nearly every transposed entry is absent: the union is nearly twice A
        assert len(se) > 1.9 * s.nnz - s.Count


def _with_zero_sums_put_back(s, H):
    """problems.symmetric_part's result H with a stored 0.0 wherever A or A^T stores an entry that H dropped."""
    import scipy.sparse as sp

    A, Hm = s.to_scipy().tocoo(), H.to_scipy().tocoo()
    zeros = np.zeros(2 * A.nnz)
    full = sp.coo_matrix((np.r_[Hm.data, zeros], (np.r_[Hm.row, A.row, A.col], np.r_[Hm.col, A.col, A.row])), shape=A.shape).tocsr()
    full.sort_indices()
    return full


@pytest.mark.parametrize("name", list(NONSYMMETRIC))
def test_symmetric_part_equals_the_host_routine_after_its_zero_sums_are_put_back(name):
    s = NONSYMMETRIC[name]()
    se, sc, sro = symmetric_part_arrays(*csr_of(s))
    full = _with_zero_sums_put_back(s, problems.symmetric_part(s))
    assert np.array_equal(full.indptr, sro) and np.array_equal(full.indices, sc) and np.array_equal(full.data, se)


def test_a_zero_sum_is_kept_and_the_host_routine_drops_it():
    s = problems.LinearSystem(np.array([2.0, -1.0, 1.0, 2.0]), np.array([0, 1, 0, 1], dtype=np.int32), np.array([0, 2, 4], dtype=np.int32),
                              np.zeros(2), np.ones(2), "skew")
    se, sc, sro = symmetric_part_arrays(*csr_of(s))
    assert se.tolist() == [2.0, 0.0, 0.0, 2.0] and sc.tolist() == [0, 1, 0, 1] and sro.tolist() == [0, 2, 4]
    H = problems.symmetric_part(s)
    assert H.nnz == 2
    full = _with_zero_sums_put_back(s, H)
    assert np.array_equal(full.indptr, sro) and np.array_equal(full.indices, sc) and np.array_equal(full.data, se)


def test_symmetric_part_of_a_symmetric_matrix_is_the_matrix_and_so_is_the_hierarchy():
    s = problems.poisson(12, 10, 8)
    e, c, ro = csr_of(s)
    se, sc, sro = symmetric_part_arrays(e, c, ro)
    assert np.array_equal(sro, ro) and np.array_equal(sc, c) and se.tobytes() == e.tobytes()
    H, G = Hierarchy(e, c, ro), HierarchySym(e, c, ro)
    assert len(H.levels) == len(G.levels) >= 3
    for L, K in zip(H.levels, G.levels):
        assert (L["map"] is None and K["map"] is None) or np.array_equal(L["map"], K["map"])
        assert np.array_equal(L["ro"], K["ro"]) and np.array_equal(L["c"], K["c"]) and L["e"].tobytes() == K["e"].tobytes()
        assert L["dinv"].tobytes() == K["dinv"].tobytes()


def test_unsorted_rows_and_duplicates_give_the_symmetric_part_of_the_sorted_and_summed_matrix():
    """Every value of the upwind stencil is a small integer and the duplicates split it 1 : 3: all sums here are exact, so the order in
    which a pair's addends arrive cannot change a bit."""
    s = NONSYMMETRIC["upwind12x10x8"]()
    ref = symmetric_part_arrays(*csr_of(s))
    for other in (reversed_rows(s), with_duplicates(s)):
        e, c, ro = csr_of(other)
        rows = np.repeat(np.arange(s.Count), np.diff(ro))
        assert np.any(np.diff(c)[np.diff(rows) == 0] <= 0)     # not ascending, or not unique
        se, sc, sro = symmetric_part_arrays(e, c, ro)
        assert np.array_equal(sro, ref[2]) and np.array_equal(sc, ref[1]) and se.tobytes() == ref[0].tobytes(), other.name


def test_small_and_one_way_matrices():
    one = problems.LinearSystem(np.array([4.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.zeros(1), np.ones(1), "one")
    se, sc, sro = symmetric_part_arrays(*csr_of(one))
    assert se.tolist() == [4.0] and sc.tolist() == [0] and sro.tolist() == [0, 1]
    se, sc, sro = symmetric_part_arrays(*csr_of(one_way_pair()))
    assert se.tolist() == [2.0, -0.5, -0.5, 3.0] and sc.tolist() == [0, 1, 0, 1] and sro.tolist() == [0, 2, 4]
    s = with_a_diagonal_only_row()
    e, c, ro = csr_of(s)
    assert ro[34] - ro[33] == 1
    se, sc, sro = symmetric_part_arrays(e, c, ro)
    assert sro[34] - sro[33] == 3 and sc[sro[33]: sro[34]].tolist() == [32, 33, 34]
    assert se[sro[33]: sro[34]].tolist() == [-0.5, 5.0, -1.5]  # half of what the neighbours store for it
    A = s.to_scipy().toarray()
    assert np.array_equal(_as_scipy(se, sc, sro).toarray(), (A + A.T) / 2)


# --------------------------------------------------------------------------- capability: what the prototype observed
def test_the_own_matching_gives_one_level_on_upwind_and_strong_central_stencils():
    for s in (upwind(20), central(20)):
        H = Hierarchy(*csr_of(s))
        print(s.name, rows_per_level(H))
        assert rows_per_level(H) == [8000]


def test_the_symmetric_matching_coarsens_them():
    G = HierarchySym(*csr_of(upwind(20)))
    print("upwind 20^3", rows_per_level(G))
    assert rows_per_level(G) == [8000, 1251, 249, 105]
    K = HierarchySym(*csr_of(central(20)))
    print("central 20^3", rows_per_level(K))
    for H in (G, K):
        assert len(H.levels) >= 2 and 4 * rows_per_level(H)[1] <= 8000
    # the level matrices are those of A itself: level 1 is sigma * P^T A P of the nonsymmetric matrix, not of its symmetric part
    e, c, ro = csr_of(upwind(20))
    L0, L1 = G.levels[0], G.levels[1]
    ge, gc, gro = galerkin(e, c, ro, L0["map"], L0["nc"], 0.5)
    assert np.array_equal(gro, L1["ro"]) and np.array_equal(gc, L1["c"]) and ge.tobytes() == L1["e"].tobytes()
    A1 = _as_scipy(L1["e"], L1["c"], L1["ro"])
    assert (A1 != A1.T).nnz > 0


def test_bicgstab_needs_fewer_bodies_behind_the_symmetric_matching_at_48_cubed():
    """48^3 central (.9, .9, .9), b ~ N(0, 1), to 1e-8 of |b|, numpy's sums in the loop.  The own matching gives one level (nuCoarse Jacobi
    sweeps); the symmetric matching four (110592 / 17522 / 3649 / 1702).  Measured with this yardstick: 25 bodies against 41 (DESIGN
    section 29).  Only the order is asserted: nobody has derived a ratio."""
    s = central(48)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    tol = 1e-8 * float(np.linalg.norm(s.b))
    e, c, ro = csr_of(s)
    t0 = time.perf_counter()
    H, G = Hierarchy(e, c, ro), HierarchySym(e, c, ro)
    own = pbicgstab_oracle(s, H.apply, tol=tol, total=np.sum)
    sym = pbicgstab_oracle(s, G.apply, tol=tol, total=np.sum)
    print(f"48^3 central (.9,.9,.9): own {rows_per_level(H)} {own['iteration']} bodies, symmetric {rows_per_level(G)} {sym['iteration']} bodies, "
          f"{time.perf_counter() - t0:.1f} s")
    assert own["status"] == sym["status"] == _lib.OK
    assert max(own["true_residual"], sym["true_residual"]) <= 1.001 * tol
    assert len(H.levels) == 1 and len(G.levels) >= 3
    assert sym["iteration"] < own["iteration"]


# --------------------------------------------------------------------------- the library without a device
def test_exports_and_python_surface(hiplib):
    for name in ("MgSetupAggregationEx", "MgStrength", "MgcgSymmetricPart"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgStrength(None) == 0
    from conjugategradient_amd import amg

    assert callable(amg.symmetric_part_gpu) and "zero" in amg.symmetric_part_gpu.__doc__
    assert amg.STRENGTHS == {"own": 0, "symmetric": 1}
    assert inspect.signature(amg.ConjugateGradientAmgGpu.__init__).parameters["strength"].default == "own"
    # a wrong word is refused before anything is created (no device is needed to see it)
    with pytest.raises(_lib.MgcgError, match="strength 'both'"):
        amg.ConjugateGradientAmgGpu(10, 7, 0, 10, 1e-8, strength="both")


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    values, offsets, short = _VectorHead(None, 28, -1, b""), _VectorHead(None, 11, -1, b""), _VectorHead(None, 10, -1, b"")
    out = _VectorHead(None, 56, -1, b"")
    ve, vo, vs, vout = C.addressof(values), C.addressof(offsets), C.addressof(short), C.addressof(out)

    def setup(strength, blas=h, sparse=h, e=ve, r=vo, c=ve, passes=3):
        L.MgcgClearLastError()
        mg = L.MgSetupAggregationEx(blas, sparse, e, r, c, 28, 10, 3, passes, 0.25, 64, 0.8, 1, 4, 0.5, strength)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return mg, msg

    for strength in (-1, 2, 7):
        mg, msg = setup(strength)
        assert not mg and f"MgSetupAggregationEx: strength {strength}, must be 0" in msg, msg
    # the arguments it shares with MgSetupAggregation are refused as there, under its own name, whatever the strength
    for strength in (0, 1):
        for kw in (dict(blas=None), dict(sparse=None), dict(e=None), dict(r=None), dict(c=None)):
            mg, msg = setup(strength, **kw)
            assert not mg and "MgSetupAggregationEx: null handle" in msg, (kw, msg)
        mg, msg = setup(strength, r=vs)
        assert not mg and "matrix vectors too small" in msg
        mg, msg = setup(strength, passes=5)
        assert not mg and "passes 5, must be 1 .. 4" in msg

    def part(blas=h, sparse=h, e=ve, r=vo, c=ve, nnz=28, count=10, oe=vout, orow=vo, oc=vout, capacity=56):
        L.MgcgClearLastError()
        got = L.MgcgSymmetricPart(blas, sparse, e, r, c, nnz, count, oe, orow, oc, capacity)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return got, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(e=None), dict(r=None), dict(c=None), dict(oe=None), dict(orow=None), dict(oc=None),
               dict(oe=None, oc=None)):
        got, msg = part(**kw)
        assert got == -1 and "MgcgSymmetricPart: null handle" in msg, (kw, msg)
    for kw in (dict(r=vs), dict(nnz=29), dict(count=11)):
        got, msg = part(**kw)
        assert got == -1 and "matrix vectors too small" in msg, (kw, msg)
    # a capacity that the output vectors do not hold, and output offsets shorter than count + 1
    for kw in (dict(capacity=57), dict(oe=ve), dict(oc=ve), dict(orow=vs)):
        got, msg = part(**kw)
        assert got == -1 and "output vectors too small" in msg, (kw, msg)
    got, msg = part(capacity=-1)
    assert got == -1 and "outCapacity -1" in msg
    big = _VectorHead(None, 2 ** 31 - 1, -1, b"")
    got, msg = part(e=C.addressof(big), c=C.addressof(big), nnz=2 ** 30)
    assert got == -1 and "exceeds INT_MAX" in msg, msg
    got, msg = part(count=0)
    assert got == -1 and "bad parameters" in msg
