"""Jacobi-preconditioned CG for general CSR matrices (``MgcgJacobiSetup`` / ``SolveJacobi``).

The geometric V-cycle only serves 5/7-point grids; every other matrix -- the reference's three driver matrices, anything a caller
brings -- gets the diagonal preconditioner here.  It is the call ``solve(A, b, cg_tag, jacobi_precond)`` that the reference's ViennaCL
front-end keeps commented out behind its hand-written loop (Mgcg/ViennaCL/Mgcg/ComputerGpu.cpp).

``ConjugateGradientJacobiGpu`` has ``ConjugateGradientSingleGpu``'s class surface.  ``Initialize()`` also extracts and checks the
diagonal (a row without a positive, finite stored diagonal raises ``MgcgError`` there, before any solve); ``Solve(trace=)`` is one
native call.  No arithmetic happens in this module.
"""
from __future__ import annotations

import numpy as np

from ._lib import MgcgError, check, lib
from .solver import ConjugateGradientSingleGpu, VectorDouble


def jacobi_setup(cusparse, vectorElements, vectorRowOffsets, vectorColumnIndeces, elementsCount, countForDevice, offsetForDevice, vectorDinv):
    """dinv = 1 / diag(A) for the local rows; raises MgcgError naming the first row without a usable diagonal.
    Sizes are checked here first (ValueError), before the library is touched."""
    elementsCount, countForDevice, offsetForDevice = int(elementsCount), int(countForDevice), int(offsetForDevice)
    if elementsCount < 0 or countForDevice < 0 or offsetForDevice < 0:
        raise ValueError("jacobi_setup: negative size")
    if vectorElements.size < elementsCount or vectorColumnIndeces.size < elementsCount:
        raise ValueError(f"jacobi_setup: the matrix vectors hold fewer than {elementsCount} entries")
    if vectorRowOffsets.size < countForDevice + 1:
        raise ValueError(f"jacobi_setup: the row offsets hold {vectorRowOffsets.size} entries, {countForDevice + 1} are needed")
    if vectorDinv.size < countForDevice:
        raise ValueError(f"jacobi_setup: the dinv vector holds {vectorDinv.size} entries, the matrix has {countForDevice} local rows")
    st = lib().MgcgJacobiSetup(cusparse, vectorElements.Ptr, vectorRowOffsets.Ptr, vectorColumnIndeces.Ptr,
                               elementsCount, countForDevice, offsetForDevice, vectorDinv.Ptr)
    if st != 0:
        check("MgcgJacobiSetup")
        raise MgcgError(f"MgcgJacobiSetup failed with status {st}")


def check_system_shapes(A, x, b, count):
    """A is a CSR matrix of `count` rows whose arrays agree with its offsets; x and b have `count` entries (ValueError otherwise)."""
    if A is None:
        raise ValueError("no matrix: load() a system or set A first")
    ro = np.asarray(A.RowOffsets)
    if ro.shape != (count + 1,):
        raise ValueError(f"RowOffsets has shape {ro.shape}, expected ({count + 1},)")
    if ro[0] != 0 or (np.diff(ro) < 0).any():
        raise ValueError("RowOffsets must start at 0 and not decrease")
    nnz = int(ro[count])
    if np.asarray(A.Elements).ndim != 1 or np.asarray(A.ColumnIndeces).ndim != 1 or len(A.Elements) < nnz or len(A.ColumnIndeces) < nnz:
        raise ValueError(f"Elements / ColumnIndeces must be vectors of at least {nnz} entries")
    for name, v in (("x", x), ("b", b)):
        if np.asarray(v).shape != (count,):
            raise ValueError(f"{name} has shape {np.asarray(v).shape}, expected ({count},)")


class ConjugateGradientJacobiGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu with M = diag(A): same constructor, members, ``Iteration`` / ``Residual`` and
    ``ApplicationException`` behaviour; the stop rules test the true residual."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.vectorDinv = VectorDouble(count)
        self._ready = False

    def Dispose(self):
        self._dispose_vectors("vectorDinv")
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                     int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def Solve(self, trace: bool = False):
        if not self._ready:
            raise MgcgError("ConjugateGradientJacobiGpu.Solve: Initialize() has not set the diagonal up")
        self._native_solve("SolveJacobi", "Jacobi-preconditioned CG", trace, work=(self.vectorDinv.Ptr,))
