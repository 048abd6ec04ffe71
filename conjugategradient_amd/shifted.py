"""Multi-shift CG: (A + shifts[j] I) x_j = b for 1 .. 8 shifts >= 0 from one CG recurrence on A (``SolveShifted``).

A regularisation path, several implicit time steps 1/dt or the poles of a rational approximation need the same matrix and right-hand
side under k different diagonal shifts.  Krylov spaces are shift-invariant, so one recurrence yields every shifted iterate: each
iteration reads the matrix once and updates all k columns in one fused vector pass, where a caller would otherwise build k shifted
matrices and run k solves.  The base system is not solved unless the shift 0 is listed.

``ConjugateGradientShiftedGpu`` has ``ConjugateGradientSingleGpu``'s class surface; ``x`` is a (k, count) array after ``Read()`` (the
initial guess is always 0), ``Iteration``, ``Residual`` and ``status`` hold one entry per shift.  One rank, no preconditioner.  No
arithmetic happens in this module.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .jacobi import check_system_shapes
from .solver import ApplicationException, ConjugateGradientGpu, ConjugateGradientSingleGpu, VectorDouble, VectorInt, _ptr


def check_shifts(shifts) -> np.ndarray:
    """shifts as a float64 vector of 1 .. 8 finite entries >= 0, or ValueError."""
    try:
        a = np.array(shifts, dtype=np.float64, copy=True)
    except (TypeError, ValueError) as e:
        raise ValueError(f"shifts = {shifts!r}: not a vector of numbers") from e
    if a.ndim != 1 or not 1 <= a.shape[0] <= _lib.SHIFT_MAX_K:
        raise ValueError(f"shifts has shape {a.shape}: a call takes 1 .. {_lib.SHIFT_MAX_K} shifts")
    for j, v in enumerate(a):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"shift {j} is {v!r}: shifts must be finite and >= 0")
    return a


class ConjugateGradientShiftedGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu for the k systems (A + shifts[j] I) x_j = b: same constructor plus ``shifts``, same members;
    ``Solve`` raises ``ApplicationException`` if any column exceeds ``MaxIteration`` (``status`` says which)."""

    def __init__(self, count, maxNonZeroCount, shifts, _minIteration, _maxIteration, allowableResidual, rule=None):
        self.cublas = None
        shifts = check_shifts(shifts)
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or int(count) < 1:
            raise ValueError(f"count = {count!r}: at least one row")
        self._count = n = int(count)
        ConjugateGradientGpu.__init__(self, n, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual)
        _lib.require_gpu()
        self.rule = rule
        self.shifts = shifts
        self.k = k = int(shifts.shape[0])
        self.cublas = self.CreateBlas()
        self.cusparse = self.CreateSparse()
        self.matDescr = self.CreateMatDescr()
        self.vectorA = VectorDouble(n * maxNonZeroCount)
        self.vectorColumnIndeces = VectorInt(n * maxNonZeroCount)
        self.vectorRowOffsets = VectorInt(n + 1)
        self.vectorX = VectorDouble(k * n)              # column j at [j * n, (j + 1) * n)
        self.vectorShiftedP = VectorDouble(k * n)
        self.vectorB, self.vectorAp, self.vectorP, self.vectorR = (VectorDouble(n) for _ in range(4))
        self.X = np.zeros((k, n), dtype=np.float64)
        self.Iteration = np.zeros(k, dtype=np.int32)
        self.Residual = np.zeros(k, dtype=np.float64)
        self.status = np.zeros(k, dtype=np.int32)
        self.trace = None

    @property
    def Count(self) -> int:
        return self._count                        # (the base class reads it off x, which is (k, count) here after Read())

    def Dispose(self):
        if getattr(self, "vectorShiftedP", None) is not None:
            self.vectorShiftedP.Dispose()
            self.vectorShiftedP = None
        if getattr(self, "cublas", None):
            super().Dispose()

    def Initialize(self):
        """Uploads A and b; the initial guess in ``x`` is not used (every column starts from 0)."""
        check_system_shapes(self.A, self.b, self.b, self.Count)          # (x is an output here: b stands in for it)
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        self.vectorA.CopyFrom(self.A.Elements, nonzeroCount)
        self.vectorColumnIndeces.CopyFrom(self.A.ColumnIndeces, nonzeroCount)
        self.vectorRowOffsets.CopyFrom(self.A.RowOffsets, self.Count + 1)
        self.vectorB.CopyFrom(self.b, self.Count)

    def Solve(self, trace: bool = False):
        k = self.k
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        rule = _lib.RULE_NATIVE if self.rule is None else self.rule
        cap = max(self.MaxIteration, self.MinIteration) + 8 if trace else 0
        tr = np.zeros((k, max(cap, 1))) if trace else None
        iteration, residual, status = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.int32)
        L = lib()
        st = L.SolveShifted(self.cublas, self.cusparse, self.matDescr,
                            self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                            self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr, self.vectorShiftedP.Ptr,
                            nonzeroCount, self.Count, k, _ptr(self.shifts),
                            self.AllowableResidual, self.MinIteration, self.MaxIteration, rule,
                            _ptr(iteration), _ptr(residual), _ptr(status), _ptr(tr) if trace else None, cap)
        if st == _lib.ERROR:
            check("SolveShifted")
            raise MgcgError("SolveShifted failed")
        self.Iteration, self.Residual, self.status = iteration, residual, status
        if trace:
            self.trace = [tr[j, : iteration[j] + 1].copy() for j in range(k)]
        L.MgcgClearLastError()
        if st == _lib.NONFINITE:
            raise MgcgError("SolveShifted: a column broke down (the matrix is not positive definite, or a scalar is not finite)")
        if st == _lib.MAXIT_EXCEEDED:
            raise ApplicationException(f"multi-shift CG: a column did not converge within MaxIteration={self.MaxIteration}")

    def Read(self):
        self.vectorX.CopyTo(self.X.reshape(-1), self.k * self.Count)
        self.x = self.X
