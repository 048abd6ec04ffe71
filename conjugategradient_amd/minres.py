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

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .jacobi import check_system_shapes, jacobi_setup
from .solver import ApplicationException, ConjugateGradientSingleGpu, VectorDouble, _ptr


class MinimalResidualGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu on the MINRES loop: same constructor (plus ``shift``), members, ``Iteration`` / ``Residual`` and
    ``ApplicationException`` behaviour, for symmetric matrices of any inertia."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, shift=0.0):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError("MinimalResidualGpu: the max-norm rule (RULE_HANDMADECL) is not supported")
        if not math.isfinite(float(shift)):
            raise ValueError("MinimalResidualGpu: the shift must be finite")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.shift = float(shift)
        self.TrueResidual = float("nan")
        self.vectorW1 = VectorDouble(count)
        self.vectorW2 = VectorDouble(count)
        self._ready = False

    def Dispose(self):
        for name in ("vectorW1", "vectorW2"):
            if getattr(self, name, None) is not None:
                getattr(self, name).Dispose()
                setattr(self, name, None)
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the residual trace in ``self.trace``; traceCapacity: its length when the default (room for every iteration) is not wanted."""
        if not self._ready:
            raise MgcgError("MinimalResidualGpu.Solve: Initialize() has not run")
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        iteration, residual, true = C.c_int(0), C.c_double(0.0), C.c_double(float("nan"))
        rule = _lib.RULE_NATIVE if self.rule is None else self.rule
        cap = (max(self.MaxIteration, self.MinIteration) + 8 if traceCapacity is None else int(traceCapacity)) if trace else 0
        tr = np.zeros(max(cap, 1)) if trace else None
        L = lib()
        st = L.SolveMinres(self.cublas, self.cusparse, self.matDescr,
                           self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                           self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr,
                           self.vectorW1.Ptr, self.vectorW2.Ptr,
                           nonzeroCount, self.Count, self.shift,
                           self.AllowableResidual, self.MinIteration, self.MaxIteration, rule,
                           C.byref(iteration), C.byref(residual), C.byref(true), _ptr(tr) if trace else None, cap)
        self.Iteration, self.Residual, self.TrueResidual, self.status = iteration.value, residual.value, true.value, st
        if trace:
            self.trace = tr[: min(self.Iteration + 1, cap)].copy()
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            raise ApplicationException(f"MINRES did not converge within MaxIteration={self.MaxIteration}")
        if st != _lib.OK:
            check("SolveMinres")
            raise MgcgError(f"SolveMinres failed with status {st}")

    def ReadResidual(self) -> np.ndarray:
        """The true residual b - (A - shift I) x that the last Solve()'s closing product left in its work vector."""
        r = np.empty(self.Count)
        self.vectorR.CopyTo(r, self.Count, 0)
        return r


class MinimalResidualJacobiGpu(MinimalResidualGpu):
    """MinimalResidualGpu with M = diag(A) (SolveMinresJacobi): same constructor and members.  ``Initialize()`` also extracts and checks
    the diagonal (a row without a positive, finite stored diagonal raises ``MgcgError`` there).

    What the stop rule judges: ``Residual``, the trace and the rule's test are the residual in the M^-1 norm, sqrt(r . M^-1 r), which is
    the quantity preconditioned MINRES minimises; ``TrueResidual`` remains the plain 2-norm || b - (A - shift I) x ||_2 of the closing
    product.  A caller who needs the 2-norm below a level looks there."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, shift=0.0):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule, shift=shift)
        self.vectorDinv = VectorDouble(count)
        self.vectorR1 = VectorDouble(count)

    def Dispose(self):
        for name in ("vectorDinv", "vectorR1"):
            if getattr(self, name, None) is not None:
                getattr(self, name).Dispose()
                setattr(self, name, None)
        super().Dispose()

    def Initialize(self):
        super().Initialize()
        self._ready = False
        jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                     int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        if not self._ready:
            raise MgcgError("MinimalResidualJacobiGpu.Solve: Initialize() has not set the diagonal up")
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        iteration, residual, true = C.c_int(0), C.c_double(0.0), C.c_double(float("nan"))
        rule = _lib.RULE_NATIVE if self.rule is None else self.rule
        cap = (max(self.MaxIteration, self.MinIteration) + 8 if traceCapacity is None else int(traceCapacity)) if trace else 0
        tr = np.zeros(max(cap, 1)) if trace else None
        L = lib()
        st = L.SolveMinresJacobi(self.cublas, self.cusparse, self.matDescr,
                                 self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                                 self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr, self.vectorR1.Ptr,
                                 self.vectorW1.Ptr, self.vectorW2.Ptr, self.vectorDinv.Ptr,
                                 nonzeroCount, self.Count, self.shift,
                                 self.AllowableResidual, self.MinIteration, self.MaxIteration, rule,
                                 C.byref(iteration), C.byref(residual), C.byref(true), _ptr(tr) if trace else None, cap)
        self.Iteration, self.Residual, self.TrueResidual, self.status = iteration.value, residual.value, true.value, st
        if trace:
            self.trace = tr[: min(self.Iteration + 1, cap)].copy()
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            raise ApplicationException(f"Jacobi-preconditioned MINRES did not converge within MaxIteration={self.MaxIteration}")
        if st != _lib.OK:
            check("SolveMinresJacobi")
            raise MgcgError(f"SolveMinresJacobi failed with status {st}")
