"""Mixed-precision CG: an fp32 recurrence corrected by fp64 reliable updates (``MgcgMixedSetup`` / ``SolveMixed`` / ``CsrMVFloat``).

The CG loop is bound by memory traffic; in fp32 an iteration on a 7-point matrix moves 100 bytes per row where the fp64 loop moves
168.  ``SolveMixed`` runs the recurrence in fp32 and, in every fourth iteration when the residual has dropped by a factor of ten or
the stop rule would fire, recomputes the true residual ``b - A x`` in fp64 and folds the fp32 partial solution into the fp64 iterate.
The search direction is kept, so the iteration count stays close to the fp64 loop's; ``x`` is fp64-accurate and the stop test is made
on a true fp64 residual.  include/MgcgGpu.h has the operation order.

``ConjugateGradientMixedGpu`` has ``ConjugateGradientSingleGpu``'s class surface.  ``Initialize()`` also converts the matrix values
(a value beyond the fp32 range raises ``MgcgError`` naming its row, before any solve); ``Solve(trace=)`` is one native call.  No
arithmetic happens in this module.
"""
from __future__ import annotations

import ctypes as C

from ._lib import MgcgError, check, lib
from .jacobi import check_system_shapes
from .solver import ConjugateGradientSingleGpu, VectorDouble


def mixed_setup(cusparse, vectorElements, vectorRowOffsets, vectorColumnIndeces, elementsCount, count, vectorElements32) -> bool:
    """elements32 = (float)elements; returns whether every value converted without rounding.  Raises MgcgError naming the first
    row with a value that is not finite as a float.  Sizes are checked here first (ValueError), before the library is touched."""
    elementsCount, count = int(elementsCount), int(count)
    if elementsCount < 0 or count < 0:
        raise ValueError("mixed_setup: negative size")
    if vectorElements.size < elementsCount or vectorColumnIndeces.size < elementsCount:
        raise ValueError(f"mixed_setup: the matrix vectors hold fewer than {elementsCount} entries")
    if vectorRowOffsets.size < count + 1:
        raise ValueError(f"mixed_setup: the row offsets hold {vectorRowOffsets.size} entries, {count + 1} are needed")
    if vectorElements32.size < (elementsCount + 1) // 2:
        raise ValueError(f"mixed_setup: the elements32 vector holds {vectorElements32.size} doubles, {elementsCount} floats need {(elementsCount + 1) // 2}")
    exact = C.c_int(0)
    st = lib().MgcgMixedSetup(cusparse, vectorElements.Ptr, vectorRowOffsets.Ptr, vectorColumnIndeces.Ptr, elementsCount, count,
                              vectorElements32.Ptr, C.byref(exact))
    if st != 0:
        check("MgcgMixedSetup")
        raise MgcgError(f"MgcgMixedSetup failed with status {st}")
    return bool(exact.value)


class ConjugateGradientMixedGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu with the fp32 inner loop: same constructor, members, ``Iteration`` / ``Residual`` (always a true
    fp64 residual) and ``ApplicationException`` behaviour, plus ``ReliableUpdates`` (updates of the last solve) and ``Exact`` (the
    matrix values are fp32 numbers).  The max-norm rule is not available."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.vectorElements32 = VectorDouble((count * maxNonZeroCount + 1) // 2)
        self.ReliableUpdates = 0
        self.Exact = False
        self._ready = False

    def Dispose(self):
        self._dispose_vectors("vectorElements32")
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        self.Exact = mixed_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                                 int(self.A.RowOffsets[self.Count]), self.Count, self.vectorElements32)
        self._ready = True

    def Solve(self, trace: bool = False):
        if not self._ready:
            raise MgcgError("ConjugateGradientMixedGpu.Solve: Initialize() has not converted the matrix")
        self._native_solve("SolveMixed", "mixed-precision CG", trace, work=(self.vectorElements32.Ptr,), third=("ReliableUpdates", 0))
