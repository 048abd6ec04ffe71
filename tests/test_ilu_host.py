"""Multicolour ILU(0) (MgSetupIlu0, ConjugateGradientIluGpu) on the host side, no GPU needed: the numpy yardstick of tests/test_gpu_ilu.py
lives here.

``IluFactor`` is the contract of include/MgcgGpu.h (MgSetupIlu0) stated in np.float64: the checks in the header's order, the colouring of
tests/test_gs_host.py, the order by (colour, row), B = P (A + shift diag(A)) P^T with sorted rows, the IKJ factor colour by colour with every
product rounded before its subtraction, and the two passes with every row summed serially in stored order (``row_sums``).  The HIP set-up
and application must EQUAL it.

Iterations to a relative 1e-8, N(0,1) right-hand side (seed 1), every sum of the loop serial, measured here
(``test_ilu_cuts_the_iterations_of_plain_cg`` prints them and asserts the inequality):

    system                      plain CG      multicolour ILU(0) CG
    poisson(16, 16, 16)            62                 30
    permuted(poisson 12^3, 7)      48                 23
"""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import (Hierarchy, _VectorHead, _raw, csr_of, diagonal_first, dominant_graph, graph_laplacian, irregular_maps, one_way, permuted,
                                 serial_dot)
from tests.test_gs_host import banded, colouring
from tests.test_mixed_host import row_sums

U = 2.0 ** -53


# --------------------------------------------------------------------------- the yardstick
def _slices(start, length):
    """The positions start[0] .. start[0] + length[0] - 1, start[1] .. one after the other, and the offsets of the pieces."""
    length = np.asarray(length, dtype=np.int64)
    offsets = np.r_[0, np.cumsum(length)]
    return np.repeat(np.asarray(start, dtype=np.int64) - offsets[:-1], length) + np.arange(int(offsets[-1])), offsets


class IluFactor:
    """ValueError with the library's words ("row 3 is empty", ...) where MgSetupIlu0 refuses, in its order."""

    def __init__(self, e, c, ro, shift=0.0):
        ro = np.asarray(ro, dtype=np.int64)
        n = len(ro) - 1
        if ro[0] != 0:
            raise ValueError(f"rowOffsets[0] is {int(ro[0])}, must be 0")
        if (np.diff(ro) < 0).any():
            raise ValueError(f"row {int(np.nonzero(np.diff(ro) < 0)[0].min())}: the row offsets descend")
        nnz = int(ro[-1])
        e, c = np.asarray(e, dtype=np.float64)[:nnz], np.asarray(c, dtype=np.int64)[:nnz]
        rows = np.repeat(np.arange(n), np.diff(ro))
        outside = (c < 0) | (c >= n)
        if outside.any():
            raise ValueError(f"row {int(rows[outside].min())} stores a column outside [0, {n})")
        if (np.diff(ro) == 0).any():
            raise ValueError(f"row {int(np.nonzero(np.diff(ro) == 0)[0].min())} is empty")
        has = np.zeros(n, dtype=bool)
        has[rows[c == rows]] = True
        if not has.all():
            raise ValueError(f"row {int(np.nonzero(~has)[0].min())} stores no diagonal entry")
        try:
            colour, self.rounds = colouring(c, ro)
        except ValueError as err:
            raise ValueError(f"level 0, {err}:") from None
        self.n, self.nnz, self.shift, self.colour = n, nnz, float(shift), colour
        # the order: new index = position in the list sorted by (colour, row)
        self.rowOf = np.lexsort((np.arange(n), colour))
        newOf = np.empty(n, dtype=np.int64)
        newOf[self.rowOf] = np.arange(n)
        self.colourOffsets = np.r_[0, np.cumsum(np.bincount(colour, minlength=int(colour.max()) + 1))]
        # B: rows in the new order, every row sorted by new column (ties by stored position: duplicates come out adjacent)
        brow, bcol = newOf[rows], newOf[c]
        order = np.lexsort((np.arange(nnz), bcol, brow))
        value = e.copy()
        scaled = shift * e[c == rows]
        value[c == rows] = e[c == rows] + scaled                      # a_ii + shift * a_ii, the product rounded first
        self.e, self.c, brow = value[order], bcol[order], brow[order]
        self.ro = np.r_[0, np.cumsum(np.bincount(brow, minlength=n))]
        key = brow * n + self.c
        twice = np.nonzero(key[1:] == key[:-1])[0]
        if len(twice):
            raise ValueError(f"row {int(self.rowOf[brow[twice]].min())} stores a column twice")
        self.diag = np.nonzero(self.c == brow)[0]
        self.B = self.e.copy()
        self._factor(key)
        self.pivots = self.e[self.diag]
        # per colour: the CSR of the parts left and right of the diagonal
        self.lower, self.upper = [], []
        for q in range(len(self.colourOffsets) - 1):
            R = np.arange(self.colourOffsets[q], self.colourOffsets[q + 1])
            k, lo = _slices(self.ro[R], self.diag[R] - self.ro[R])
            self.lower.append((R, self.e[k], self.c[k], lo))
            k, uo = _slices(self.diag[R] + 1, self.ro[R + 1] - self.diag[R] - 1)
            self.upper.append((R, self.e[k], self.c[k], uo))

    def _factor(self, key):
        n, v, c, ro, diag = self.n, self.e, self.c, self.ro, self.diag
        self.pinv = pinv = np.zeros(n)
        with np.errstate(all="ignore"):
            for q in range(len(self.colourOffsets) - 1):
                R = np.arange(self.colourOffsets[q], self.colourOffsets[q + 1])
                left = diag[R] - ro[R]
                for step in range(int(left.max()) if len(R) else 0):
                    A = R[left > step]
                    p = ro[A] + step
                    k = c[p]
                    l = v[p] * pinv[k]
                    v[p] = l
                    count = ro[k + 1] - diag[k] - 1
                    at, _ = _slices(diag[k] + 1, count)                    # the entries (k, j), j > k, of every row's k
                    want = np.repeat(A, count) * n + c[at]
                    pos = np.minimum(np.searchsorted(key, want), len(key) - 1)
                    found = key[pos] == want                              # row i stores column j
                    product = np.repeat(l, count)[found] * v[at[found]]
                    v[pos[found]] = v[pos[found]] - product
                pivot = v[diag[R]]
                bad = (pivot == 0.0) | ~np.isfinite(pivot)
                if bad.any():
                    first = np.nonzero(bad)[0][0]                         # (the colour's rows ascend in the old numbering too)
                    raise ValueError(f"row {int(self.rowOf[R[first]])}: the pivot is {pivot[first]:g}")
                pinv[R] = 1.0 / pivot

    def colours(self):
        return len(self.colourOffsets) - 1

    def pivot_range(self):
        return float(self.pivots.min()), float(self.pivots.max())

    def apply(self, r):
        r = np.asarray(r, dtype=np.float64)
        y, t, z = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        for R, e, c, ro in self.lower:
            y[R] = r[self.rowOf[R]] - row_sums(e, c, ro, y)
        for R, e, c, ro in self.upper[::-1]:
            res = y[R] - row_sums(e, c, ro, t)
            t[R] = self.pinv[R] * res
            z[self.rowOf[R]] = t[R]
        return z

    def triangles(self):
        """(L with its unit diagonal, U) as scipy matrices in the new order."""
        import scipy.sparse as sp

        rows = np.repeat(np.arange(self.n), np.diff(self.ro))
        low = self.c < rows
        L = sp.csr_matrix((self.e[low], (rows[low], self.c[low])), shape=(self.n, self.n)) + sp.identity(self.n, format="csr")
        return L.tocsr(), sp.csr_matrix((self.e[~low], (rows[~low], self.c[~low])), shape=(self.n, self.n))


class IluLoop:
    """What Hierarchy.pcg needs: the matrix as levels[0] and apply()."""
    pcg = Hierarchy.pcg

    def __init__(self, s, shift=0.0):
        e, c, ro = csr_of(s)
        self.levels = [dict(e=e, c=c, ro=ro)]
        self.factor = IluFactor(e, c, ro, shift)
        self.apply = self.factor.apply


# --------------------------------------------------------------------------- the systems of the two test files
def rows_unsorted(s):
    """Every row with its diagonal first and the rest in descending column order: no row sorted."""
    e, c, ro = csr_of(s)
    rows = np.repeat(np.arange(s.Count), np.diff(ro))
    order = np.lexsort((-c, c != rows, rows))
    return _raw(s, e[order], c[order], ro, s.name + "-unsorted")


def coarse_level_of_irregular_maps():
    """Level 1 of the hierarchy tests/test_gs_host.py colours with 26 colours: 46 rows, more than 20 entries a row."""
    s = dominant_graph(10, 3)
    L = Hierarchy(*csr_of(s), maps=irregular_maps(s.Count)).levels[1]
    n = len(L["ro"]) - 1
    out = problems.LinearSystem(L["e"].copy(), L["c"].astype(np.int32), L["ro"].astype(np.int32), np.zeros(n), np.ones(n), "irregular-level-1")
    return out


def _stencils():
    cd = dict(c=(0.5, 0.25, 0.0))
    return {
        "poisson6x5x4": lambda: problems.poisson(6, 5, 4),
        "poisson6x5x4-permuted": lambda: permuted(problems.poisson(6, 5, 4), 7),
        "convdiff6x5x4": lambda: problems.convection_diffusion(6, 5, 4, **cd),
        "upwind6x5x4": lambda: problems.convection_diffusion(6, 5, 4, c=(2.0, 1.0, 0.5), upwind=True),
    }


SYSTEMS = dict(_stencils())
SYSTEMS.update({name + "-unsorted": (lambda make=make: rows_unsorted(make())) for name, make in _stencils().items()})
SYSTEMS.update({name + "-diagonal-first": (lambda make=make: diagonal_first(make())) for name, make in _stencils().items()})
SYSTEMS.update({
    "banded-200-12": lambda: banded(200, 12),
    "irregular-level-1": coarse_level_of_irregular_maps,
    "rows-1": lambda: problems.poisson(1, 1, 1),
    "rows-2": lambda: problems.poisson(2, 1, 1),
    "rows-3": lambda: problems.poisson(3, 1, 1),
    "rows-5": lambda: problems.poisson(5, 1, 1),
})
SHIFTS = (0.0, 0.1)
SYMMETRIC = [name for name in SYSTEMS if not name.startswith(("convdiff", "upwind"))]


# --------------------------------------------------------------------------- the factor
def _at(M, i, j):
    """The entries (i[q], j[q]) of a scipy matrix as an array (also of none)."""
    return np.asarray(M[i, j], dtype=np.float64).ravel() if len(i) else np.zeros(0)


def test_the_factor_by_hand_on_a_path_of_four_rows():
    """tridiag(-1, 2, -1): the colours are 1 0 1 0 (tests/test_gs_host.py runs the rule by hand), so the order is old rows 1 3 | 0 2.
        new row 0 (old 1): columns old 0 1 2 = new 2 0 3:  (0: 2) (2: -1) (3: -1)          pivot 2
        new row 1 (old 3): columns old 2 3 = new 3 1:      (1: 2) (3: -1)                  pivot 2
        new row 2 (old 0): (0: -1) (2: 2):  l = -1 * 0.5 = -0.5;  row 0 holds (2: -1): 2 - (-0.5 * -1) = 1.5;  row 0's (3: -1) finds no
                           column 3 here: the fill is dropped.                             pivot 1.5
        new row 3 (old 2): (0: -1) (1: -1) (3: 2):  l = -0.5, row 0's (3: -1): 2 - 0.5 = 1.5;  l = -0.5, row 1's (3: -1): 1.5 - 0.5 = 1
                                                                                          pivot 1"""
    ro, c = np.array([0, 2, 5, 8, 10]), np.array([0, 1, 0, 1, 2, 1, 2, 3, 2, 3])
    e = np.array([2.0, -1, -1, 2, -1, -1, 2, -1, -1, 2])
    F = IluFactor(e, c, ro)
    assert F.colour.tolist() == [1, 0, 1, 0] and F.rowOf.tolist() == [1, 3, 0, 2] and F.colourOffsets.tolist() == [0, 2, 4]
    assert F.ro.tolist() == [0, 3, 5, 7, 10] and F.c.tolist() == [0, 2, 3, 1, 3, 0, 2, 0, 1, 3] and F.diag.tolist() == [0, 3, 6, 9]
    assert F.B.tolist() == [2.0, -1, -1, 2, -1, -1, 2, -1, -1, 2]
    assert F.e.tolist() == [2.0, -1, -1, 2, -1, -0.5, 1.5, -0.5, -0.5, 1.0]
    assert F.pinv.tolist() == [0.5, 0.5, 1.0 / 1.5, 1.0] and F.pivot_range() == (1.0, 2.0) and F.colours() == 2
    # one application by hand, r = (1, 2, 3, 4) in the old order = (2, 4, 1, 3) in the new one
    y = [2.0, 4.0, 1.0 - (-0.5 * 2.0), 3.0 - ((0.0 + -0.5 * 2.0) + -0.5 * 4.0)]
    t3 = 1.0 * y[3]
    t2 = (1.0 / 1.5) * y[2]
    t1 = 0.5 * (y[1] - (-1.0 * t3))
    t0 = 0.5 * (y[0] - ((0.0 + -1.0 * t2) + -1.0 * t3))
    assert F.apply(np.array([1.0, 2, 3, 4])).tolist() == [t2, t0, t3, t1]
    # the shift: the diagonal is a + shift * a with the product rounded first
    G = IluFactor(e, c, ro, shift=0.1)
    assert G.B[G.diag].tolist() == [2.0 + 0.1 * 2.0] * 4


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_l_times_u_equals_b_on_the_pattern_within_the_rounding_of_the_recurrence(name, shift):
    """|(L U)_ij - b_ij| <= (2 m + 2) 2^-53 (|b_ij| + sum_k |l_ik| |u_kj|) for every stored (i, j), m the terms of the sum: m products and m
    subtractions, the reciprocal and the product with it; nothing measured.  (The check's own sum is scipy's: within m 2^-53 of the same
    magnitude, inside the same bound's slack only because the bound counts every operation at a full unit; the observed ratio is printed.)"""
    F = IluFactor(*csr_of(SYSTEMS[name]()), shift=shift)
    L, Um = F.triangles()
    rows = np.repeat(np.arange(F.n), np.diff(F.ro))
    product = _at(L @ Um, rows, F.c)
    magnitude = _at(abs(L) @ abs(Um), rows, F.c)
    ones = lambda M: (M != 0).astype(np.float64)
    terms = _at(ones(L) @ ones(Um), rows, F.c)
    bound = (2 * terms + 2) * U * (np.abs(F.B) + magnitude)
    error = np.abs(product - F.B)
    print(f"{name} shift {shift}: colours {F.colours()}, pivots {F.pivot_range()}, max error / bound {float((error / bound).max()):.3f}")
    assert (error <= bound).all()
    assert F.colours() == int(F.colour.max()) + 1 and np.array_equal(np.sort(F.rowOf), np.arange(F.n))
    assert all((np.diff(F.c[F.ro[i]:F.ro[i + 1]]) > 0).all() for i in range(F.n))


@pytest.mark.parametrize("name", SYMMETRIC)
def test_on_a_symmetric_matrix_u_is_the_pivot_scaled_transpose_of_l(name):
    """Exactly, U = D L^T.  In floating point u_ij and l_ji * u_ii are two evaluations of one recurrence whose terms l_ik u_kj and
    l_jk u_ki = (l_ik u_kk) l_jk agree to the roundings of l and of the products: per entry the (2 m + 2) 2^-53 (|b_ij| + sum |l_ik| |u_kj|)
    of the test above, once for each side, and the entries it reads carry the same from the colour before -- a chain no longer than the
    colours.  The systems are diagonally dominant, |l| < 1, so inherited errors do not grow: the bound is 2 x colours x that figure."""
    F = IluFactor(*csr_of(SYSTEMS[name]()))
    L, Um = F.triangles()
    rows = np.repeat(np.arange(F.n), np.diff(F.ro))
    up = F.c > rows
    i, j = rows[up], F.c[up]
    mirrored = _at(L, j, i) * F.pivots[i]
    magnitude = _at(abs(L) @ abs(Um), i, j)
    terms = _at((L != 0).astype(np.float64) @ (Um != 0).astype(np.float64), i, j)
    bound = 2 * F.colours() * (2 * terms + 2) * U * (np.abs(F.B[up]) + magnitude)
    assert (np.abs(F.e[up] - mirrored) <= bound).all()


# --------------------------------------------------------------------------- refusals
def _csr(rows):
    """CSR arrays of a list of rows, each a list of (column, value)."""
    ro = np.r_[0, np.cumsum([len(r) for r in rows])]
    return (np.array([v for r in rows for _, v in r], dtype=np.float64), np.array([c for r in rows for c, _ in r], dtype=np.int64), ro)


REFUSED = {
    "no-diagonal": (lambda: _csr([[(0, 2.0), (1, -1.0)], [(0, -1.0)], [(2, 1.0)]]), "row 1 stores no diagonal entry"),
    "duplicate": (lambda: _csr([[(0, 2.0), (1, -1.0)], [(0, -0.5), (1, 2.0), (0, -0.5)]]), "row 1 stores a column twice"),
    "empty-row": (lambda: _csr([[(0, 2.0)], [], [(2, 1.0)]]), "row 1 is empty"),
    "zero-pivot": (lambda: _csr([[(0, 1.0), (1, 1.0)], [(0, 1.0), (1, 1.0)]]), "the pivot is 0"),
    "column-outside": (lambda: _csr([[(0, 2.0), (2, 1.0)], [(1, 1.0)]]), "row 0 stores a column outside [0, 2)"),
    "descending": (lambda: (np.ones(3), np.array([0, 1, 1]), np.array([0, 2, 1, 3])), "row 1: the row offsets descend"),
    "unsymmetric-pattern": (lambda: csr_of(one_way(graph_laplacian(10, 3))), "level 0, row"),
    "65-colours": (lambda: (np.where(np.eye(65, dtype=bool), 100.0, -1.0).ravel(), np.tile(np.arange(65), 65), np.arange(66) * 65), "level 0, row"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_the_yardstick_refuses_what_the_header_refuses(name):
    make, words = REFUSED[name]
    with pytest.raises(ValueError) as err:
        IluFactor(*make())
    assert words in str(err.value), str(err.value)


def test_the_zero_pivot_is_the_second_one_of_the_matrix_of_ones():
    """[[1, 1], [1, 1]]: whichever row comes first has pivot 1, l = 1 * 1, and the second pivot is 1 - 1 * 1 = 0."""
    e, c, ro = REFUSED["zero-pivot"][0]()
    colour, _ = colouring(c, ro)
    second = int(np.lexsort((np.arange(2), colour))[1])
    with pytest.raises(ValueError, match=f"^row {second}: the pivot is 0$"):
        IluFactor(e, c, ro)
    F = IluFactor(e, c, ro, shift=0.5)                              # the remedy: ILU(0) of A + 0.5 D
    assert F.pivot_range()[0] > 0.0


# --------------------------------------------------------------------------- the loop
def _iterations(loop, s):
    out = loop.pcg(np.asarray(s.b), tol=1e-8 * float(np.linalg.norm(s.b)), dot=serial_dot)
    assert out["status"] == _lib.OK
    assert np.linalg.norm(s.b - s.to_scipy() @ out["x"]) < 2e-8 * float(np.linalg.norm(s.b))
    return out["iteration"]


class _Plain:
    pcg = Hierarchy.pcg

    def __init__(self, s):
        e, c, ro = csr_of(s)
        self.levels = [dict(e=e, c=c, ro=ro)]

    def apply(self, r):
        return r.copy()


@pytest.mark.parametrize("name", ["poisson16", "poisson12-permuted"])
def test_ilu_cuts_the_iterations_of_plain_cg(name):
    s = problems.poisson(16, 16, 16) if name == "poisson16" else permuted(problems.poisson(12, 12, 12), 7)
    s.b = np.random.default_rng(1).standard_normal(s.Count)
    loop = IluLoop(s)
    plain, ilu = _iterations(_Plain(s), s), _iterations(loop, s)
    print(f"{name}: colours {loop.factor.colours()}, pivots {loop.factor.pivot_range()}; iterations: plain {plain}, ILU(0) {ilu}")
    assert loop.factor.pivot_range()[0] > 0.0
    assert ilu < plain


# --------------------------------------------------------------------------- the library without a device
EXPORTS = ("MgSetupIlu0", "MgIsIlu", "MgIluColours", "MgIluPivotRange", "MgIluSetupMs", "MgIluCopyFactor")


def test_exports_and_python_surface(hiplib):
    for name in EXPORTS:
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3
    assert hiplib.MgIsIlu(None) == 0
    import conjugategradient_amd
    from conjugategradient_amd import amg, ilu

    assert "ilu" in conjugategradient_amd.__all__
    assert issubclass(ilu.ConjugateGradientIluGpu, amg.ConjugateGradientAmgGpu)
    for member in ("Apply", "Solve", "SolveMinres", "SolveBicgstab", "SolveGmres", "colours", "pivot_range", "factor"):
        assert callable(getattr(ilu.ConjugateGradientIluGpu, member))
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "MgcgGpu.h")).read()
    for name in EXPORTS:
        assert f" {name}(" in header, name


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    values, offsets, short = _VectorHead(None, 28, -1, b""), _VectorHead(None, 11, -1, b""), _VectorHead(None, 10, -1, b"")
    ve, vo, vs = C.addressof(values), C.addressof(offsets), C.addressof(short)

    def setup(blas=h, sparse=h, e=ve, r=vo, c=ve, nnz=28, count=10, shift=0.0):
        L.MgcgClearLastError()
        mg = L.MgSetupIlu0(blas, sparse, e, r, c, nnz, count, shift)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return mg, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(e=None), dict(r=None), dict(c=None)):
        mg, msg = setup(**kw)
        assert not mg and "MgSetupIlu0: null handle" in msg, (kw, msg)
    for kw in (dict(count=0), dict(count=-3), dict(nnz=-1)):
        mg, msg = setup(**kw)
        assert not mg and "MgSetupIlu0: bad parameters" in msg, (kw, msg)
    for kw in (dict(r=vs), dict(e=vs), dict(c=vs), dict(count=11), dict(nnz=29)):
        mg, msg = setup(**kw)
        assert not mg and "MgSetupIlu0: matrix vectors too small" in msg, (kw, msg)
    for shift in (-0.1, float("inf"), float("nan")):
        mg, msg = setup(shift=shift)
        assert not mg and "MgSetupIlu0: shift" in msg and "must be finite and >= 0" in msg, (shift, msg)
    # the queries on what is no ILU handle
    lo, hi = C.c_double(0.0), C.c_double(0.0)
    for call, who in ((lambda: L.MgIluColours(None), "MgIluColours"), (lambda: L.MgIluPivotRange(None, C.byref(lo), C.byref(hi)), "MgIluPivotRange"),
                      (lambda: L.MgIluCopyFactor(None, None, None, None, None, None), "MgIluCopyFactor"), (lambda: L.MgIluSetupMs(None, None), "MgIluSetupMs")):
        L.MgcgClearLastError()
        assert call() == -1
        assert f"{who}: the handle is not an ILU(0) factor" in _lib.last_error()
        L.MgcgClearLastError()
    assert L.MgIsIlu(h) == 0                                     # zeroed memory standing for a hierarchy: no factor behind it
