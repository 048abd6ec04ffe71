"""Restarted GMRES(m) (``SolveGmres``, ``SolveGmresJacobi``): nonsymmetric systems A x = b, the robust member of the family.

``bicgstab`` solves the same systems with fixed storage and fewer bytes per product, but its residual can peak many orders above || b ||,
it ends MGCG_NONFINITE where convection dominates, and on a badly conditioned matrix the residual it carries drifts from b - A x.  GMRES
(Saad and Schultz) minimises the residual over the Krylov space itself: the judged residual never increases, the method cannot break down
on a nonsingular matrix, and every restart recomputes r = b - A x by a product.  It pays with ``m + 1`` basis vectors and with traffic that
grows with the step's place in its cycle: slower per product than BiCGStab and BiCGStab(l) -- use it where they break down, stagnate or
drift.

``GeneralizedMinimalResidualGpu(count, maxNonZeroCount, minIteration, maxIteration, allowableResidual, rule=None, m=20, orth=2)`` has
``BiConjugateGradientStabLGpu``'s class surface: ``Iteration``, ``MinIteration``, ``MaxIteration`` and the trace count Arnoldi steps (one
product each), ``Residual`` is the rotated estimate of || b - A x ||_2, ``TrueResidual`` that norm itself from one closing product, and
``ReadResidual()`` returns that vector.  ``m`` (1 .. 32) is the restart length, ``orth`` (1 or 2) the number of classical Gram-Schmidt
passes per step.  ``GeneralizedMinimalResidualJacobiGpu`` is the same with M = diag(A) as right preconditioner.  One rank.  The V-cycle as right
preconditioner, in Saad's flexible form (``SolveGmresMg``), is the method ``SolveGmres(trace=False, hierarchy=None, m=20, orth=2)`` of
``multigrid.ConjugateGradientMgGpu``, ``amg.ConjugateGradientAmgGpu`` and ``ssor.ConjugateGradientSsorGpu``.

The max-norm stop rule is not supported.  No arithmetic happens in this module.
"""
from __future__ import annotations

from .bicgstab import OneWorkVectorGpu

MAX_M = 32


class GeneralizedMinimalResidualGpu(OneWorkVectorGpu):
    """BiConjugateGradientStabGpu on the GMRES(m) loop (SolveGmres): same members, ``TrueResidual``, ``ReadResidual()``, trace and exceptions;
    iterations count Arnoldi steps.  One work vector of ``m + 1`` slices (one more with the diagonal) holds the basis: it is sized for the
    object's ``m`` and allocated again, larger, by the first ``Solve()`` after ``m`` was raised.  The library checks ``m``, ``orth`` and the
    vector's size; a value it refuses leaves the object usable with another."""

    _export = "SolveGmres"
    _what = "GMRES(m)"

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, m=20, orth=2):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.m, self.orth = int(m), int(orth)
        self._ensure_work(self._slices())

    def _slices(self):
        return min(max(int(self.m), 1), MAX_M) + 1 + self._slices_more

    def _work_arguments(self):
        self._ensure_work(self._slices())
        return (self.vectorWork.Ptr, *self._more_vectors(), int(self.m), int(self.orth))


class GeneralizedMinimalResidualJacobiGpu(GeneralizedMinimalResidualGpu):
    """GeneralizedMinimalResidualGpu with M = diag(A) as right preconditioner (SolveGmresJacobi); ``Initialize()`` also extracts and checks
    the diagonal, as ``BiConjugateGradientStabJacobiGpu`` does."""

    _export = "SolveGmresJacobi"
    _what = "Jacobi-preconditioned GMRES(m)"
    _jacobi = True
