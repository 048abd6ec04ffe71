"""Shared-subspace block CG: k (1..8) right-hand sides on one matrix in ONE block Krylov space (SolveBlockKrylov; O'Leary's block CG in
Dubrulle's breakdown-free form).  Where ``ConjugateGradientBlockGpu`` runs k independent recurrences that share the matrix pass, here
every column minimises over the union of the k Krylov spaces: all columns converge in fewer iterations and stop together.

Dependent or zero initial residual columns (two equal right-hand sides, b_j = 0, an x_j that already solves its system) are a breakdown:
``Solve`` raises ``MgcgError`` and x is left as it was; fall back to ``ConjugateGradientBlockGpu``, whose columns are independent.

One rank, no preconditioner, plain CSR, the four 2-norm stop rules.  Like solver.py this module holds no arithmetic: every flop happens
in the HIP library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .block import ConjugateGradientBlockGpu
from .solver import ApplicationException, _ptr


class ConjugateGradientBlockKrylovGpu(ConjugateGradientBlockGpu):
    """``ConjugateGradientBlockGpu``'s surface (``load``, ``Initialize``, ``Solve(trace=)``, ``Read``) on the shared-subspace loop.
    ``Iteration`` is ONE number, the common counter; ``Residual`` and ``status`` (also ``Status``) are length-k arrays of the last
    iteration; with ``trace=True`` ``trace`` is a list of k per-column residual traces of equal length."""

    def __init__(self, count, maxNonZeroCount, k, _minIteration, _maxIteration, allowableResidual, rule=None):
        if rule is not None and int(rule) == _lib.RULE_HANDMADECL:
            raise ValueError("the max-norm rule (RULE_HANDMADECL) is not supported by the shared-subspace loop: the residual block is never formed")
        super().__init__(count, maxNonZeroCount, k, _minIteration, _maxIteration, allowableResidual, rule)
        self.Iteration = 0
        self.status = self.Status

    def Solve(self, trace: bool = False):
        k, n = self.k, self.Count
        nonzeroCount = int(self.A.RowOffsets[n])
        it = C.c_int(0)
        res = np.zeros(k, dtype=np.float64)
        status = np.zeros(k, dtype=np.int32)
        cap = max(self.MaxIteration, self.MinIteration) + 8 if trace else 0
        tr = np.zeros(max(k * cap, 1)) if trace else None
        L = lib()
        st = L.SolveBlockKrylov(self.cublas, self.cusparse, self.matDescr,
                                self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                                self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr,
                                nonzeroCount, n, k,
                                self.AllowableResidual, self.MinIteration, self.MaxIteration, self.rule,
                                C.byref(it), _ptr(res), _ptr(status), _ptr(tr) if trace else None, cap)
        if st == _lib.ERROR:
            check("SolveBlockKrylov")
            raise MgcgError("SolveBlockKrylov failed")
        self.Iteration, self.Residual, self.Status = int(it.value), res, status
        self.status = status
        if st == _lib.NONFINITE:
            self.trace = None
            check("SolveBlockKrylov")
            raise MgcgError("SolveBlockKrylov: breakdown")
        if trace:
            self.trace = [tr[j * cap: j * cap + min(self.Iteration + 1, cap)].copy() for j in range(k)]
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            bad = [j for j in range(k) if status[j] == _lib.MAXIT_EXCEEDED]
            raise ApplicationException(f"block CG did not converge within MaxIteration={self.MaxIteration} in columns {bad}")
