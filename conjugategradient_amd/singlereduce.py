"""Single-reduction CG (``SolveSingleReduce``): Chronopoulos-Gear CG, one global sum and two launches per iteration.

The same Krylov method as ``ConjugateGradientSingleGpu`` / ``ConjugateGradientJacobiGpu`` with the matrix product moved in front of both
dot products, so that an iteration is the product plus ONE fused vector pass (one small reduce, one all-reduce and the pass on several
ranks: ``ConjugateGradientRankGpu.SolveSingleReduce``).  It costs one more vector and 8 bytes per row more pass traffic than the plain
loop: a loop for latency-bound systems and for ranks, not for systems whose iteration is memory traffic.

``ConjugateGradientSingleReduceGpu`` has ``ConjugateGradientSingleGpu``'s class surface.  ``jacobi=True`` adds the diagonal
preconditioner (``Initialize()`` then extracts and checks the diagonal, as ``ConjugateGradientJacobiGpu`` does); the max-norm stop rule
is not supported.  After ``Solve()``, ``ReadResidual()`` returns the recurrence residual.  No arithmetic happens in this module.
"""
from __future__ import annotations

from . import _lib
from ._lib import MgcgError
from .jacobi import check_system_shapes, jacobi_setup
from .solver import ConjugateGradientSingleGpu, VectorDouble


class ConjugateGradientSingleReduceGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu on the single-reduction loop: same constructor (plus ``jacobi``), members, ``Iteration`` / ``Residual``
    and ``ApplicationException`` behaviour; the stop rules test the true residual.  ``ReadResidual()`` returns the recurrence residual r
    that the last Solve() left in its work vector."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, jacobi=False):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError("ConjugateGradientSingleReduceGpu: the max-norm rule (RULE_HANDMADECL) is not supported")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.jacobi = bool(jacobi)
        self.vectorS = VectorDouble(count)
        self.vectorDinv = VectorDouble(count) if self.jacobi else None
        self._ready = False

    def Dispose(self):
        self._dispose_vectors("vectorS", "vectorDinv")
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        if self.jacobi:
            jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                         int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the residual trace in ``self.trace``; traceCapacity: its length when the default (room for every iteration) is not wanted."""
        if not self._ready:
            raise MgcgError("ConjugateGradientSingleReduceGpu.Solve: Initialize() has not run")
        self._native_solve("SolveSingleReduce", "single-reduction CG", trace, traceCapacity=traceCapacity,
                           work=(self.vectorS.Ptr, self.vectorDinv.Ptr if self.jacobi else None))
