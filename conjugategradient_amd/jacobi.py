"""Jacobi-preconditioned CG for general CSR matrices (``MgcgJacobiSetup`` / ``SolveJacobi``).

The geometric V-cycle only serves 5/7-point grids; every other matrix -- the reference's three driver matrices, anything a caller
brings -- gets the diagonal preconditioner here.  It is the call ``solve(A, b, cg_tag, jacobi_precond)`` that the reference's ViennaCL
front-end keeps commented out behind its hand-written loop (Mgcg/ViennaCL/Mgcg/ComputerGpu.cpp).

``ConjugateGradientJacobiGpu`` has ``ConjugateGradientSingleGpu``'s class surface.  ``Initialize()`` also extracts and checks the
diagonal (a row without a positive, finite stored diagonal raises ``MgcgError`` there, before any solve); ``Solve(trace=)`` is one
native call.  No arithmetic happens in this module.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .solver import ApplicationException, ConjugateGradientSingleGpu, VectorDouble, _ptr


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
        if getattr(self, "vectorDinv", None) is not None:
            self.vectorDinv.Dispose()
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
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        iteration, residual = C.c_int(0), C.c_double(0.0)
        rule = _lib.RULE_NATIVE if self.rule is None else self.rule
        cap = max(self.MaxIteration, self.MinIteration) + 8 if trace else 0
        tr = np.zeros(max(cap, 1)) if trace else None
        L = lib()
        st = L.SolveJacobi(self.cublas, self.cusparse, self.matDescr,
                           self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                           self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr, self.vectorDinv.Ptr,
                           nonzeroCount, self.Count,
                           self.AllowableResidual, self.MinIteration, self.MaxIteration, rule,
                           C.byref(iteration), C.byref(residual), _ptr(tr) if trace else None, cap)
        self.Iteration, self.Residual, self.status = iteration.value, residual.value, st
        if trace:
            self.trace = tr[: self.Iteration + 1].copy()
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            raise ApplicationException(f"Jacobi-preconditioned CG did not converge within MaxIteration={self.MaxIteration}")
        if st != _lib.OK:
            check("SolveJacobi")
            raise MgcgError(f"SolveJacobi failed with status {st}")
