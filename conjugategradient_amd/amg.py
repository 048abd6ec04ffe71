"""Aggregation multigrid (``MgSetupAggregation`` / ``MgSetupAggregates``): the V-cycle preconditioner of ``multigrid`` for any CSR matrix.

The hierarchy is the one of ``ConjugateGradientMgGpu`` -- piecewise-constant transfer, coarse operators sigma * P^T A P, weighted Jacobi --
with the aggregates taken from the matrix graph by a deterministic parallel matching (include/MgcgGpu.h writes the algorithm out;
tests/test_amg_host.py states it in numpy) instead of 2x2x2 boxes of a grid, so the matrix needs no grid and no row order: a permuted
stencil, a mesh or particle matrix, a graph Laplacian with jumping weights.  ``aggregates`` hands the library the caller's own maps.
One GPU; ``omega`` is the caller's (omega * lambda_max(D^-1 A) < 2 keeps the preconditioner positive definite under the Jacobi smoother;
``smoother="gs"``, multicolour Gauss-Seidel, is positive definite for every 0 < omega < 2).  No arithmetic on vectors happens here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .multigrid import ConjugateGradientMgGpu
from .problems import LinearSystem
from .solver import ConjugateGradientGpu, VectorDouble, VectorInt, _ptr


SMOOTHERS = {"jacobi": 0, "gs": 1}          # MgSetSmoother's modes
STRENGTHS = {"own": 0, "symmetric": 1}      # MgSetupAggregationEx's: what the matching reads
CYCLES = {"V": 0, "K": 1}                   # MgSetCycle's modes ...
INNERS = {"conjugate": 0, "minimal": 1}     # ... and the inner steps of the K-cycle


def symmetric_part_gpu(system: LinearSystem) -> LinearSystem:
    """(A + A^T) / 2 of a system's matrix formed on the device (``MgcgSymmetricPart``), with the same b, x and grid: the device counterpart
    of ``problems.symmetric_part``.  Columns ascend and appear once a row; unlike the host routine it KEEPS the sums that come to zero, as
    stored 0.0 entries (an entry >= 0 never couples in the matching, so they change no map).  Rows of A may be unsorted and hold
    duplicates."""
    _lib.require_gpu()
    L = lib()
    n, nnz = system.Count, system.nnz
    if 2 * nnz > 2 ** 31 - 1:
        raise MgcgError(f"symmetric_part_gpu: 2 x {nnz} entries exceed INT_MAX")
    blas, sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
    vectors = []
    try:
        for kind, size in ((VectorDouble, nnz), (VectorInt, n + 1), (VectorInt, nnz), (VectorDouble, 2 * nnz), (VectorInt, n + 1), (VectorInt, 2 * nnz)):
            vectors.append(kind(max(size, 1)))
        a, ro, ci, sa, sro, sci = vectors
        a.CopyFrom(np.ascontiguousarray(system.Elements[:nnz], dtype=np.float64), nnz)
        ro.CopyFrom(np.ascontiguousarray(system.RowOffsets, dtype=np.int32), n + 1)
        ci.CopyFrom(np.ascontiguousarray(system.ColumnIndeces[:nnz], dtype=np.int32), nnz)
        count = L.MgcgSymmetricPart(blas, sparse, a.Ptr, ro.Ptr, ci.Ptr, nnz, n, sa.Ptr, sro.Ptr, sci.Ptr, 2 * nnz)
        check("MgcgSymmetricPart")
        if count < 0:
            raise MgcgError("MgcgSymmetricPart failed")
        return LinearSystem(sa.to_numpy(count), sci.to_numpy(count), sro.to_numpy(n + 1), np.array(system.x, dtype=np.float64),
                            np.array(system.b, dtype=np.float64), f"{system.name}-sym", grid=system.grid)
    finally:
        for v in vectors:
            v.Dispose()
        L.DestroyBlas(blas)
        L.DestroySparse(sparse)


def transpose_class_limits():
    """(shortMax, ldsMax) of ``MgcgCsrTranspose``: a column stored shortMax times or less is sorted by one lane in registers, one stored
    ldsMax times or less by one workgroup in LDS, a longer one by one workgroup in global memory.  Needs no GPU."""
    short, lds = C.c_int(0), C.c_int(0)
    lib().MgcgTransposeClassLimits(C.byref(short), C.byref(lds))
    return short.value, lds.value


def csr_transpose_gpu(elements, column_indices, row_offsets, columns, with_source=False):
    """A^T of a CSR matrix of ``len(row_offsets) - 1`` rows and ``columns`` columns, formed on the device (``MgcgCsrTranspose``): numpy
    arrays ``(elements, column_indices, row_offsets)`` of A^T, and the source list behind them with ``with_source`` (``source[q]`` = the
    stored position in A of entry q of A^T).  Row c of A^T holds the stored entries of column c of A by ascending stored position; values
    are bit copies.  ``elements`` None asks for the pattern alone and gives None back in its place.  Rows may be unsorted, empty and hold
    duplicates; entries beyond ``row_offsets[-1]`` are ignored."""
    _lib.require_gpu()
    L = lib()
    ro = np.ascontiguousarray(row_offsets, dtype=np.int32)
    ci = np.ascontiguousarray(column_indices, dtype=np.int32)
    rows, held, columns = len(ro) - 1, len(ci), int(columns)
    if elements is not None:
        elements = np.ascontiguousarray(elements, dtype=np.float64)
        if len(elements) != held:
            raise MgcgError(f"csr_transpose_gpu: {len(elements)} values, {held} columns")
    blas, sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
    vectors = {}
    try:
        sizes = dict(ro=(VectorInt, rows + 1), ci=(VectorInt, held), tro=(VectorInt, columns + 1), tci=(VectorInt, held))
        if elements is not None:
            sizes.update(a=(VectorDouble, held), ta=(VectorDouble, held))
        if with_source:
            sizes.update(src=(VectorInt, held))
        for key, (kind, size) in sizes.items():
            vectors[key] = kind(max(size, 1))
        vectors["ro"].CopyFrom(ro, rows + 1)
        if held:
            vectors["ci"].CopyFrom(ci, held)
            if elements is not None:
                vectors["a"].CopyFrom(elements, held)
        ptr = lambda key: vectors[key].Ptr if key in vectors else None
        count = L.MgcgCsrTranspose(blas, sparse, ptr("a"), ptr("ro"), ptr("ci"), held, rows, columns, ptr("ta"), ptr("tro"), ptr("tci"), ptr("src"))
        check("MgcgCsrTranspose")
        if count < 0:
            raise MgcgError("MgcgCsrTranspose failed")
        out = (vectors["ta"].to_numpy(max(held, 1))[:count] if elements is not None else None, vectors["tci"].to_numpy(max(held, 1))[:count],
               vectors["tro"].to_numpy(columns + 1))
        return out + (vectors["src"].to_numpy(max(held, 1))[:count],) if with_source else out
    finally:
        for v in vectors.values():
            v.Dispose()
        L.DestroyBlas(blas)
        L.DestroySparse(sparse)


def transpose_gpu(system: LinearSystem) -> LinearSystem:
    """A^T of a (square) system's matrix formed on the device (``csr_transpose_gpu``), with the same b, x and grid.  Its rows come out with
    ascending columns whatever the order of A's rows; duplicates stay apart, in stored order."""
    n, nnz = system.Count, system.nnz
    e, c, ro = csr_transpose_gpu(system.Elements[:nnz], system.ColumnIndeces[:nnz], system.RowOffsets, n)
    return LinearSystem(e, c, ro, np.array(system.x, dtype=np.float64), np.array(system.b, dtype=np.float64), f"{system.name}-T", grid=system.grid)


def multiply_class_limits():
    """(shortMax, ldsMax) of ``MgcgCsrMultiply``: a row of C of shortMax products or fewer is formed by one lane in registers, one of
    ldsMax products or fewer by one workgroup in LDS, a longer one by one workgroup in global scratch.  Needs no GPU."""
    short, lds = C.c_int(0), C.c_int(0)
    lib().MgcgMultiplyClassLimits(C.byref(short), C.byref(lds))
    return short.value, lds.value


def csr_multiply_gpu(a, b, columns):
    """C = A B of two CSR matrices formed on the device (``MgcgCsrMultiply``).  ``a`` and ``b`` are ``(elements or None, column_indices,
    row_offsets)``; A has ``len(a[2]) - 1`` rows, B has ``len(b[2]) - 1`` rows -- the columns of A -- and ``columns`` columns.  Returns
    numpy arrays ``(elements, column_indices, row_offsets)`` of C; ``elements`` None in both asks for the pattern alone and gives None back
    in its place.  Columns of C ascend and appear once a row; c_ij is the serial sum, from +0.0, of its products a_ik * b_kj in the order
    row i of A and then row k of B store them (no FMA), and a sum that comes to zero stays as a stored 0.0.  Rows may be unsorted, empty
    and hold duplicates; entries beyond ``row_offsets[-1]`` are ignored.  Two calls: the count of C, then the arrays."""
    _lib.require_gpu()
    L = lib()
    if (a[0] is None) != (b[0] is None):
        raise MgcgError("csr_multiply_gpu: the elements of a and b are given together, or neither of them")
    host = {}
    for key, (e, c, ro) in (("a", a), ("b", b)):
        host[key + "ro"] = np.ascontiguousarray(ro, dtype=np.int32)
        host[key + "ci"] = np.ascontiguousarray(c, dtype=np.int32)
        if e is not None:
            host[key + "e"] = np.ascontiguousarray(e, dtype=np.float64)
            if len(host[key + "e"]) != len(host[key + "ci"]):
                raise MgcgError(f"csr_multiply_gpu: {key}: {len(host[key + 'e'])} values, {len(host[key + 'ci'])} columns")
    rows, inner, columns = len(host["aro"]) - 1, len(host["bro"]) - 1, int(columns)
    heldA, heldB = len(host["aci"]), len(host["bci"])
    blas, sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
    vectors = {}
    try:
        for key, array in host.items():
            vectors[key] = (VectorDouble if key.endswith("e") else VectorInt)(max(len(array), 1))
            if len(array):
                vectors[key].CopyFrom(array, len(array))
        ptr = lambda key: vectors[key].Ptr if key in vectors else None
        matrices = (blas, sparse, ptr("ae"), ptr("aro"), ptr("aci"), heldA, ptr("be"), ptr("bro"), ptr("bci"), heldB, rows, inner, columns)
        count = L.MgcgCsrMultiply(*matrices, None, None, None, 0)
        check("MgcgCsrMultiply")
        if count < 0:
            raise MgcgError("MgcgCsrMultiply failed")
        room = max(int(count), 1)
        vectors["cro"], vectors["cci"] = VectorInt(rows + 1), VectorInt(room)
        if a[0] is not None:
            vectors["ce"] = VectorDouble(room)
        if L.MgcgCsrMultiply(*matrices, ptr("ce"), ptr("cro"), ptr("cci"), int(count)) != count:
            check("MgcgCsrMultiply")
            raise MgcgError("MgcgCsrMultiply failed")
        return (vectors["ce"].to_numpy(room)[:count] if a[0] is not None else None, vectors["cci"].to_numpy(room)[:count],
                vectors["cro"].to_numpy(rows + 1))
    finally:
        for v in vectors.values():
            v.Dispose()
        L.DestroyBlas(blas)
        L.DestroySparse(sparse)


def multiply_gpu(system_a: LinearSystem, system_b: LinearSystem) -> LinearSystem:
    """A B of two square systems' matrices of one size formed on the device (``csr_multiply_gpu``), with b, x and grid of the first."""
    n = system_a.Count
    if system_b.Count != n:
        raise MgcgError(f"multiply_gpu: {n} rows times {system_b.Count} rows")
    na, nb = system_a.nnz, system_b.nnz
    e, c, ro = csr_multiply_gpu((system_a.Elements[:na], system_a.ColumnIndeces[:na], system_a.RowOffsets),
                                (system_b.Elements[:nb], system_b.ColumnIndeces[:nb], system_b.RowOffsets), n)
    return LinearSystem(e, c, ro, np.array(system_a.x, dtype=np.float64), np.array(system_a.b, dtype=np.float64),
                        f"{system_a.name}*{system_b.name}", grid=system_a.grid)


class ConjugateGradientAmgGpu(ConjugateGradientMgGpu):
    """ConjugateGradientMgGpu without ``grid``: ``Apply``, ``Solve(trace=...)``, ``level_csr`` and ``level_dinv`` are the parent's.

    ``aggregates``: None (the library's matching: ``passes`` passes per level at strength threshold ``theta``, at most ``levels`` levels,
    none built from a level of ``minCoarse`` rows or fewer) or a list of per-level maps, ``aggregates[l][i]`` = the aggregate of row i of
    level l; the hierarchy then has ``len(aggregates) + 1`` levels and the last map's largest id + 1 rows on its last level.

    ``smoother``: "jacobi" (weighted Jacobi, the default) or "gs" (multicolour Gauss-Seidel, MgSetSmoother(mg, 1): an even ``nuCoarse``
    and a structurally symmetric pattern of at most 64 colours a level; symmetric positive definite for every 0 < omega < 2).  It is
    applied in ``Setup()`` after the hierarchy is built; a refusal raises MgcgError with the library's message and leaves ``self.mg`` a
    usable Jacobi hierarchy.

    ``strength``: what the library's matching reads -- "own" (the level's own matrix, the default: MgSetupAggregation) or "symmetric" (the
    symmetric part of every level's own matrix, formed on the device: MgSetupAggregationEx with strength = 1; the level matrices stay
    sigma * P^T A P of A itself).  For A != A^T, where "own" may not coarsen at all.  Ignored with ``aggregates``.

    ``cycle``: "V" (the default) or "K" (MgSetCycle(mg, 1, inner): on every level whose coarse level has a map of its own, two Krylov steps
    preconditioned by the cycle stand where the V-cycle runs one coarse cycle), with ``inner`` "conjugate" or "minimal" (residual) steps.
    It is applied in ``Setup()`` after the smoother; a refusal raises MgcgError with the library's message and leaves ``self.mg`` a usable
    V hierarchy.  The K-cycle is no fixed linear map: ``Apply``, ``Solve`` and ``SolveGmres`` take it, ``SolveMinres``, ``SolveBicgstab`` and
    ``SolveLobpcg`` raise the library's refusal."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual,
                 levels: int = 8, passes: int = 3, theta: float = 0.25, minCoarse: int = 64, omega: float = 0.8, nu: int = 1, nuCoarse: int = 4,
                 sigma: float = 0.5, aggregates=None, rule=_lib.RULE_CSHARP, smoother: str = "jacobi",
                 strength: str = "own", cycle: str = "V", inner: str = "conjugate"):
        if smoother not in SMOOTHERS:
            raise MgcgError(f"smoother {smoother!r}, must be one of {sorted(SMOOTHERS)}")
        if strength not in STRENGTHS:
            raise MgcgError(f"strength {strength!r}, must be one of {sorted(STRENGTHS)}")
        if cycle not in CYCLES:
            raise MgcgError(f"cycle {cycle!r}, must be one of {sorted(CYCLES)}")
        if inner not in INNERS:
            raise MgcgError(f"inner {inner!r}, must be one of {sorted(INNERS)}")
        self.smoother, self.strength, self.cycle, self.inner = smoother, strength, cycle, inner
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, (count, 1, 1),
                         levels=levels, omega=omega, nu=nu, nuCoarse=nuCoarse, sigma=sigma, rule=rule)
        self.passes, self.theta, self.minCoarse = int(passes), float(theta), int(minCoarse)
        self.aggregates = None if aggregates is None else [np.ascontiguousarray(m, dtype=np.int32) for m in aggregates]

    def InitializePoisson(self, grid, b_value: float = 1.0, x_value: float = 0.0):
        """The parent's device generator for the 5/7-point matrix of ``grid`` (the hierarchy is built from the matrix alone)."""
        saved, self.grid = self.grid, tuple(int(g) for g in grid)
        try:
            super().InitializePoisson(b_value, x_value)
        finally:
            self.grid = saved

    def Setup(self):
        nonzeroCount = int(self.A.RowOffsets[self.Count]) if self.A is not None else self._nnz
        L = lib()
        if self.aggregates is None and self.strength not in STRENGTHS:      # (changed after construction: refused before any call)
            raise MgcgError(f"strength {self.strength!r}, must be one of {sorted(STRENGTHS)}")
        if self.mg:
            L.MgDestroy(self.mg)
            self.mg = None
        matrix = (self.cublas, self.cusparse, self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr, nonzeroCount, self.Count)
        if self.aggregates is None and STRENGTHS[self.strength]:
            name = "MgSetupAggregationEx"
            self.mg = L.MgSetupAggregationEx(*matrix, int(self.levels_requested), self.passes, self.theta, self.minCoarse,
                                             self.omega, self.nu, self.nuCoarse, self.sigma, STRENGTHS[self.strength])
        elif self.aggregates is None:
            name = "MgSetupAggregation"
            self.mg = L.MgSetupAggregation(*matrix, int(self.levels_requested), self.passes, self.theta, self.minCoarse,
                                           self.omega, self.nu, self.nuCoarse, self.sigma)
        else:
            name = "MgSetupAggregates"
            maps = self.aggregates
            if maps and len(maps[0]) != self.Count:
                raise MgcgError(f"aggregates[0] holds {len(maps[0])} ids, the matrix has {self.Count} rows")
            rows = [self.Count] + [len(m) for m in maps[1:]] + ([int(maps[-1].max()) + 1] if maps else [])
            levelRows = np.asarray(rows, dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate(maps), dtype=np.int32) if maps else np.zeros(1, dtype=np.int32)
            self.mg = L.MgSetupAggregates(*matrix, len(rows), _ptr(levelRows), _ptr(flat), self.omega, self.nu, self.nuCoarse, self.sigma)
        check(name)
        if not self.mg:
            raise MgcgError(f"{name} returned NULL")
        self.levels = L.MgLevels(self.mg)
        if SMOOTHERS[self.smoother] and L.MgSetSmoother(self.mg, SMOOTHERS[self.smoother]) != 0:
            check("MgSetSmoother")
            raise MgcgError("MgSetSmoother failed")
        if CYCLES[self.cycle] and L.MgSetCycle(self.mg, CYCLES[self.cycle], INNERS[self.inner]) != 0:
            check("MgSetCycle")
            raise MgcgError("MgSetCycle failed")

    def UpdateValues(self, elements=None):
        """New values for the pattern the hierarchy was built from (``MgUpdateValues``): the maps, the colours and the modes stay, every
        coarse matrix and every D^-1 is formed again -- bit for bit what ``aggregates=[level_aggregates(l) ...]`` builds from the new
        values, not necessarily what the matching would choose for them.  ``elements``: a host array of the nnz values in stored order,
        which overwrites ``self.A.Elements`` and ``vectorA``; or None, for a caller who wrote ``vectorA`` on the device.  A refusal (a bad
        diagonal on some level among them) raises MgcgError with the library's message and leaves the coarse levels and D^-1 as they were."""
        nnz = int(self.A.RowOffsets[self.Count]) if self.A is not None else self._nnz
        if elements is not None:
            e = np.ascontiguousarray(elements, dtype=np.float64)
            if e.shape != (nnz,):
                raise MgcgError(f"UpdateValues: {e.size} values, the matrix has {nnz} entries")
            if self.A is not None:                          # (a new array: ``load`` may have taken the system's own, which stays the caller's)
                held = np.array(self.A.Elements, dtype=np.float64)
                held[:nnz] = e
                self.A.Elements = held
            self.vectorA.CopyFrom(e, nnz)
        status = lib().MgUpdateValues(self.mg, self.vectorA.Ptr, nnz)
        check("MgUpdateValues")
        if status != 0:
            raise MgcgError("MgUpdateValues failed")

    def update_bytes(self) -> int:
        """Device bytes of the source lists and shadow buffers of ``UpdateValues`` (0 before its first call)."""
        return int(lib().MgUpdateBytes(self.mg))

    def level_galerkin_sources(self, l: int):
        """``(sources, segment_offsets)`` of level ``l``: entry q of level ``l + 1`` is sigma times the serial sum of level l's stored entries
        ``sources[segment_offsets[q]:segment_offsets[q + 1]]`` in that order (MgcgError before the first ``UpdateValues`` and on the last level)."""
        L = lib()
        offsets = np.empty(max(int(L.MgLevelNnz(self.mg, l + 1)), 0) + 1, dtype=np.int32)
        sources = np.empty(max(int(L.MgLevelNnz(self.mg, l)), 1), dtype=np.int32)
        count = L.MgLevelCopyGalerkinSources(self.mg, l, _ptr(offsets), _ptr(sources))
        check("MgLevelCopyGalerkinSources")
        if count < 0:
            raise MgcgError("MgLevelCopyGalerkinSources failed")
        return sources[:count], offsets

    def level_colours(self, l: int) -> np.ndarray:
        """The colour of every row of level ``l`` under ``smoother="gs"`` (MgcgError under "jacobi")."""
        c = np.empty(lib().MgLevelRows(self.mg, l), dtype=np.int32)
        if lib().MgLevelCopyColours(self.mg, l, _ptr(c)) != 0:
            check("MgLevelCopyColours")
            raise MgcgError("MgLevelCopyColours failed")
        return c

    def level_aggregates(self, l: int) -> np.ndarray:
        """The map of level ``l`` to level ``l + 1`` (MgcgError on the last level)."""
        m = np.empty(lib().MgLevelRows(self.mg, l), dtype=np.int32)
        if lib().MgLevelCopyAggregates(self.mg, l, _ptr(m)) != 0:
            check("MgLevelCopyAggregates")
            raise MgcgError("MgLevelCopyAggregates failed")
        return m
