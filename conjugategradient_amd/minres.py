"""MINRES (``SolveMinres``): symmetric indefinite and shifted systems (A - shift I) x = b.

Every CG loop of this package needs a positive definite matrix and stops with ``NONFINITE`` when p.Ap <= 0.  MINRES (Paige and Saunders)
runs the same Lanczos recurrence at the same cost structure -- one product and two global sums per iteration -- for ANY symmetric matrix,
and minimises the 2-norm of the residual, which is what every stop rule here judges: on a definite matrix it never needs more iterations
than CG, and its residual trace never increases.  ``shift`` may have any sign (A - shift I for shift-and-invert with a Ritz value from
``spectrum``, a Helmholtz-type operator, a Poisson matrix with a negative shift); it costs nothing inside the loop.

``MinimalResidualGpu`` has ``ConjugateGradientSingleGpu``'s class surface.  ``Iteration``, ``Residual`` and the trace show the
recurrence's residual; ``TrueResidual`` is || b - (A - shift I) x ||_2 from one closing product, and ``ReadResidual()`` returns that
vector.  Several ranks: ``ConjugateGradientRankGpu.SolveMinres``.  The max-norm stop rule is not supported.

``MinimalResidualJacobiGpu`` is the same class on the preconditioned loop with M = diag(A) (``SolveMinresJacobi``); the V-cycle form is
``ConjugateGradientMgGpu.SolveMinres`` / ``ConjugateGradientAmgGpu.SolveMinres`` (``SolveMinresMg``), several ranks
``ConjugateGradientRankGpu.SolveMinresJacobi``.  With a preconditioner ``Iteration``, ``Residual`` and the trace show the residual in the
M^-1 norm, sqrt(r . M^-1 r) -- that is what preconditioned MINRES minimises and what the stop rule judges -- while ``TrueResidual``
remains the plain 2-norm.  No arithmetic happens in this module.
"""
from __future__ import annotations

import math

from . import _lib
from ._lib import MgcgError
from .jacobi import check_system_shapes, jacobi_setup
from .solver import ConjugateGradientSingleGpu, VectorDouble


class MinimalResidualGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu on the MINRES loop: same constructor (plus ``shift``), members, ``Iteration`` / ``Residual`` and
    ``ApplicationException`` behaviour, for symmetric matrices of any inertia.  ``ReadResidual()`` returns the true residual
    b - (A - shift I) x that the last Solve()'s closing product left in its work vector."""

    _export = "SolveMinres"
    _what = "MINRES"
    _jacobi = False                    # with M = diag(A): ``vectorDinv``, filled and checked by Initialize(), and ``vectorR1``
    _unready = "has not run"

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, shift=0.0):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError("MinimalResidualGpu: the max-norm rule (RULE_HANDMADECL) is not supported")
        if not math.isfinite(float(shift)):
            raise ValueError("MinimalResidualGpu: the shift must be finite")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.shift = float(shift)
        self.TrueResidual = float("nan")
        for name in ("vectorW1", "vectorW2") + (("vectorDinv", "vectorR1") if self._jacobi else ()):
            setattr(self, name, VectorDouble(count))
        self._ready = False

    def Dispose(self):
        self._dispose_vectors("vectorDinv", "vectorR1", "vectorW1", "vectorW2")
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        if self._jacobi:
            jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                         int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the residual trace in ``self.trace``; traceCapacity: its length when the default (room for every iteration) is not wanted."""
        if not self._ready:
            raise MgcgError(f"{type(self).__name__}.Solve: Initialize() {self._unready}")
        work = (self.vectorR1.Ptr, self.vectorW1.Ptr, self.vectorW2.Ptr, self.vectorDinv.Ptr) if self._jacobi else (self.vectorW1.Ptr, self.vectorW2.Ptr)
        self._native_solve(self._export, self._what, trace, work=work, more=(self.shift,), third=("TrueResidual", float("nan")),
                           traceCapacity=traceCapacity)


class MinimalResidualJacobiGpu(MinimalResidualGpu):
    """MinimalResidualGpu with M = diag(A) (SolveMinresJacobi): same constructor and members.  ``Initialize()`` also extracts and checks
    the diagonal (a row without a positive, finite stored diagonal raises ``MgcgError`` there).

    What the stop rule judges: ``Residual``, the trace and the rule's test are the residual in the M^-1 norm, sqrt(r . M^-1 r), which is
    the quantity preconditioned MINRES minimises; ``TrueResidual`` remains the plain 2-norm || b - (A - shift I) x ||_2 of the closing
    product.  A caller who needs the 2-norm below a level looks there."""

    _export = "SolveMinresJacobi"
    _what = "Jacobi-preconditioned MINRES"
    _jacobi = True
    _unready = "has not set the diagonal up"
