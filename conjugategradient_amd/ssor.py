"""SSOR(omega)-preconditioned CG, MINRES, BiCGStab and GMRES(m) for any CSR matrix with a structurally symmetric pattern.

The preconditioner is the one-level form of ``amg`` under the multicolour Gauss-Seidel smoother (``MgSetSmoother(mg, 1)``): no aggregates,
``nuCoarse = 2`` sweeps from zero -- one forward, one backward -- which is symmetric Gauss-Seidel in the colour order for omega = 1 and
SSOR(omega) otherwise, symmetric positive definite on a symmetric positive definite matrix for every 0 < omega < 2.  What a matrix that will
not coarsen (no negative couplings) gets between the diagonal (``jacobi``) and a hierarchy.  ``Solve``, ``SolveMinres``, ``SolveBicgstab``,
``SolveGmres`` and ``Apply`` are the parent's; no arithmetic happens here.
"""
from __future__ import annotations

from . import _lib
from .amg import ConjugateGradientAmgGpu


class ConjugateGradientSsorGpu(ConjugateGradientAmgGpu):
    """ConjugateGradientAmgGpu with ``aggregates=[]``, ``nuCoarse=2``, ``smoother="gs"``; ``omega`` is the relaxation factor."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, omega: float = 1.0, rule=_lib.RULE_CSHARP):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, levels=1, omega=omega, nu=1, nuCoarse=2,
                         aggregates=[], rule=rule, smoother="gs")
