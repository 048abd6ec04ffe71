"""Chebyshev-preconditioned CG (``SolveChebyshev``): a polynomial preconditioner for any CSR matrix.

z = p_m(A) r, the Chebyshev polynomial for an interval [lambdaMin, lambdaMax] that holds the part of the spectrum worth damping, needs only
the matrix product and no global sum.  One CG iteration then carries ``degree`` products and still two global sums (one all-reduce pair on
ranks: ``ConjugateGradientRankGpu.SolveChebyshev``), and a step of the polynomial is one launch: fewer iterations, fewer reduction points
per product, for systems whose iteration is launch latency or all-reduces, not for those that are memory traffic.

``ConjugateGradientChebyshevGpu`` has ``ConjugateGradientSingleReduceGpu``'s class surface plus ``degree``, ``bounds`` and ``eigRatio``.
With ``bounds=None`` ``Initialize()`` takes lambdaMax from ``MgcgGershgorinBound`` (rigorous) and sets lambdaMin = lambdaMax / ``eigRatio``;
``lambdaMin`` / ``lambdaMax`` say what was used.  A caller with a ``spectrum.py`` estimate passes ``bounds`` -- with a margin (5-10 %) on a
Lanczos lambdaMax, which approaches the true value from BELOW: an upper bound under the spectrum makes the preconditioner indefinite
and the solve stops with ``MGCG_NONFINITE``.  A lambdaMin above the true one only costs iterations.  ``jacobi=True`` lets the polynomial
act on D^-1 A (the bounds are then bounds of D^-1 A).  The max-norm stop rule is not supported.  No arithmetic on vectors happens here.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib
from ._lib import MgcgError, check, lib
from .jacobi import check_system_shapes, jacobi_setup
from .solver import ConjugateGradientSingleGpu, VectorDouble


def gershgorin_bound(cusparse, vectorElements, vectorRowOffsets, vectorColumnIndeces, elementsCount, countForDevice, offsetForDevice, vectorDinv=None):
    """max_i sum_j |a_ij| (times dinv_i) over the local rows: an upper bound of the spectrum of A (of D^-1 A)."""
    bound = C.c_double(0.0)
    st = lib().MgcgGershgorinBound(cusparse, vectorElements.Ptr, vectorRowOffsets.Ptr, vectorColumnIndeces.Ptr,
                                   int(elementsCount), int(countForDevice), int(offsetForDevice),
                                   vectorDinv.Ptr if vectorDinv is not None else None, C.byref(bound))
    if st != 0:
        check("MgcgGershgorinBound")
        raise MgcgError(f"MgcgGershgorinBound failed with status {st}")
    return bound.value


def check_bounds(degree, lambdaMin, lambdaMax):
    """What SolveChebyshev refuses, said before the library is touched (ValueError)."""
    if not 1 <= int(degree) <= 16:
        raise ValueError(f"degree {degree}, must be 1 .. 16")
    if not (math.isfinite(lambdaMin) and math.isfinite(lambdaMax) and 0.0 < lambdaMin < lambdaMax):
        raise ValueError(f"the bounds ({lambdaMin}, {lambdaMax}) must be finite with 0 < lambdaMin < lambdaMax")


class ConjugateGradientChebyshevGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu on the Chebyshev-preconditioned loop: same constructor (plus ``degree``, ``jacobi``, ``bounds``,
    ``eigRatio``), members, ``Iteration`` / ``Residual`` and ``ApplicationException`` behaviour; the stop rules test the true residual.
    ``ReadResidual()`` returns the recurrence residual r that the last Solve() left in its work vector."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, degree=4, jacobi=False, bounds=None, eigRatio=30.0):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError("ConjugateGradientChebyshevGpu: the max-norm rule (RULE_HANDMADECL) is not supported")
        if not 1 <= int(degree) <= 16:
            raise ValueError(f"ConjugateGradientChebyshevGpu: degree {degree}, must be 1 .. 16")
        if bounds is not None:
            check_bounds(degree, float(bounds[0]), float(bounds[1]))
        elif not (math.isfinite(eigRatio) and eigRatio > 1.0):
            raise ValueError(f"ConjugateGradientChebyshevGpu: eigRatio {eigRatio}, must be finite and > 1")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.degree, self.jacobi, self.bounds, self.eigRatio = int(degree), bool(jacobi), bounds, float(eigRatio)
        self.lambdaMin = self.lambdaMax = None
        self.vectorZ, self.vectorZ2, self.vectorD = VectorDouble(count), VectorDouble(count), VectorDouble(count)
        self.vectorDinv = VectorDouble(count) if self.jacobi else None
        self._ready = False

    def Dispose(self):
        self._dispose_vectors("vectorZ", "vectorZ2", "vectorD", "vectorDinv")
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        if self.jacobi:
            jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces, nonzeroCount, self.Count, 0, self.vectorDinv)
        if self.bounds is None:
            self.lambdaMax = gershgorin_bound(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces, nonzeroCount, self.Count, 0, self.vectorDinv)
            self.lambdaMin = self.lambdaMax / self.eigRatio
        else:
            self.lambdaMin, self.lambdaMax = float(self.bounds[0]), float(self.bounds[1])
        check_bounds(self.degree, self.lambdaMin, self.lambdaMax)
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the residual trace in ``self.trace``; traceCapacity: its length when the default (room for every iteration) is not wanted."""
        if not self._ready:
            raise MgcgError("ConjugateGradientChebyshevGpu.Solve: Initialize() has not run")
        self._native_solve("SolveChebyshev", "Chebyshev-preconditioned CG", trace, traceCapacity=traceCapacity,
                           work=(self.vectorDinv.Ptr if self.jacobi else None, self.vectorZ.Ptr, self.vectorZ2.Ptr, self.vectorD.Ptr),
                           more=(self.degree, self.lambdaMin, self.lambdaMax))
