"""LSQR (``MgcgSolveLsqr``): least squares min || A x - b ||_2 for a rectangular CSR matrix, optionally damped.

Every other solver of this package takes a square matrix and drives b - A x to zero.  LSQR (Paige and Saunders) takes ANY CSR matrix --
more rows than columns or fewer, rank deficient, square and nonsymmetric or singular -- and any right-hand side, consistent or not, and
minimises || A x - b ||^2 + damp^2 || x ||^2; where the minimiser is not unique it tends to the one of minimum norm.  It never forms A^T A.
What the stop rule judges is the estimate of || A^T (b - A x) - damp^2 x ||_2, which tends to zero whether or not the system is
consistent; the residual norm itself does not.

``LeastSquaresGpu`` keeps A and A^T on the device: ``Initialize()`` uploads A and forms A^T there with ``MgcgCsrTranspose`` -- nothing
makes a host round trip -- so the transposed product is the ordinary gather product, deterministic and without float atomics.
``Iteration``, ``Residual`` and the trace show the judged estimate, ``ResidualNorm`` the estimate of the (damped) residual norm;
``TrueResidual`` = || b - A x ||_2 and ``TrueNormalResidual`` = || A^T (b - A x) - damp^2 x ||_2 come from two closing products, whose
vectors ``ReadResidual()`` (rows) and ``ReadNormalResidual()`` (columns) return.  x always starts from 0: a caller with a guess x0
passes b - A x0 and adds x0 back.  One rank.  No arithmetic happens in this module.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .solver import ApplicationException, ConjugateGradientGpu, SparseMatrix, VectorDouble, VectorInt, _ptr


class LeastSquaresGpu(ConjugateGradientGpu):
    """min || A x - b ||^2 + damp^2 || x ||^2 for A of ``rows`` x ``columns`` with at most ``maxNonZeroCount`` stored entries per row.
    Members as the other classes': ``A`` (a SparseMatrix), ``b`` (rows entries), ``x`` (columns entries: the result; its content
    before the call is ignored), ``Iteration`` / ``Residual`` and ``ApplicationException`` past MaxIteration."""

    DEVICE_ID = 0

    def __init__(self, rows, columns, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, damp=0.0):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError("LeastSquaresGpu: the max-norm rule (RULE_HANDMADECL) is not supported")
        if not (math.isfinite(float(damp)) and float(damp) >= 0.0):
            raise ValueError("LeastSquaresGpu: damp must be finite and >= 0")
        if int(rows) < 1 or int(columns) < 1:
            raise ValueError("LeastSquaresGpu: rows and columns must be >= 1")
        super().__init__(int(columns), maxNonZeroCount, _minIteration, _maxIteration, allowableResidual)
        self.Rows, self.Columns = int(rows), int(columns)
        self.b = np.zeros(self.Rows, dtype=np.float64)
        self.rule, self.damp = rule, float(damp)
        self.ResidualNorm = self.TrueResidual = self.TrueNormalResidual = float("nan")
        self.trace, self.status, self._ready = None, 0, False
        _lib.require_gpu()
        self.cublas = self.CreateBlas()
        self.cusparse = self.CreateSparse()
        self.matDescr = self.CreateMatDescr()
        capacity = max(self.Rows * int(maxNonZeroCount), 1)
        self.vectorA, self.vectorColumnIndeces, self.vectorRowOffsets = VectorDouble(capacity), VectorInt(capacity), VectorInt(self.Rows + 1)
        self.vectorAT, self.vectorColumnIndecesT, self.vectorRowOffsetsT = VectorDouble(capacity), VectorInt(capacity), VectorInt(self.Columns + 1)
        self.vectorB, self.vectorU, self.vectorQ = (VectorDouble(self.Rows) for _ in range(3))
        self.vectorX, self.vectorV, self.vectorW, self.vectorT = (VectorDouble(self.Columns) for _ in range(4))

    _vectors = ("vectorA", "vectorColumnIndeces", "vectorRowOffsets", "vectorAT", "vectorColumnIndecesT", "vectorRowOffsetsT",
                "vectorB", "vectorU", "vectorQ", "vectorX", "vectorV", "vectorW", "vectorT")

    def Dispose(self):
        self._dispose_vectors(*self._vectors)
        if getattr(self, "cublas", None):
            lib().DestroyBlas(self.cublas)
            lib().DestroySparse(self.cusparse)
            lib().DestroyMatDescr(self.matDescr)
            self.cublas = None

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass

    def load(self, system):
        """Take A and b from a ``problems.LeastSquaresSystem`` (or anything with its members)."""
        columns = int(getattr(system, "Columns", self.Columns))
        rows = int(np.asarray(system.RowOffsets).shape[0]) - 1
        if (rows, columns) != (self.Rows, self.Columns):
            raise MgcgError(f"LeastSquaresGpu.load: the system is {rows} x {columns}, this object {self.Rows} x {self.Columns}")
        self.A = SparseMatrix.from_system(system)
        self.b[:] = system.b
        return self

    def Initialize(self):
        """Upload A and b, and form A^T on the device (MgcgCsrTranspose: a matrix it refuses raises MgcgError with its message here)."""
        self._ready = False
        ro = self.A.RowOffsets
        if ro.shape[0] != self.Rows + 1 or self.b.shape[0] != self.Rows:
            raise MgcgError(f"LeastSquaresGpu.Initialize: {ro.shape[0] - 1} rows of A and {self.b.shape[0]} entries of b, this object has {self.Rows} rows")
        nnz = int(ro[self.Rows])
        if nnz > self.vectorA.size or nnz > min(self.A.Elements.shape[0], self.A.ColumnIndeces.shape[0]):
            raise MgcgError(f"LeastSquaresGpu.Initialize: {nnz} stored entries, room for {self.vectorA.size}")
        if nnz:
            self.vectorA.CopyFrom(self.A.Elements, nnz)
            self.vectorColumnIndeces.CopyFrom(self.A.ColumnIndeces, nnz)
        self.vectorRowOffsets.CopyFrom(ro, self.Rows + 1)
        self.vectorB.CopyFrom(self.b, self.Rows)
        count = lib().MgcgCsrTranspose(self.cublas, self.cusparse, self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                                       nnz, self.Rows, self.Columns, self.vectorAT.Ptr, self.vectorRowOffsetsT.Ptr, self.vectorColumnIndecesT.Ptr, None)
        check("MgcgCsrTranspose")
        if count < 0:
            raise MgcgError("MgcgCsrTranspose failed")
        self._nnz = nnz
        self._ready = True

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the trace of the judged estimate in ``self.trace``; traceCapacity: its length when the default (room for every
        iteration) is not wanted.  Stores every output, THEN raises ApplicationException past MaxIteration and MgcgError for every other
        status but MGCG_OK."""
        if not self._ready:
            raise MgcgError("LeastSquaresGpu.Solve: Initialize() has not run")
        it = C.c_int(0)
        res, norm, true, normal = (C.c_double(float("nan")) for _ in range(4))
        cap = (max(self.MaxIteration, self.MinIteration) + 8 if traceCapacity is None else int(traceCapacity)) if trace else 0
        tr = np.zeros(max(cap, 1)) if trace else None
        L = lib()
        st = L.MgcgSolveLsqr(self.cublas, self.cusparse, self.matDescr,
                         self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                         self.vectorAT.Ptr, self.vectorRowOffsetsT.Ptr, self.vectorColumnIndecesT.Ptr,
                         self.vectorX.Ptr, self.vectorB.Ptr, self.vectorU.Ptr, self.vectorV.Ptr, self.vectorW.Ptr, self.vectorQ.Ptr, self.vectorT.Ptr,
                         self._nnz, self.Rows, self.Columns, self.damp,
                         self.AllowableResidual, self.MinIteration, self.MaxIteration, self._rule(),
                         C.byref(it), C.byref(res), C.byref(norm), C.byref(true), C.byref(normal), _ptr(tr) if trace else None, cap)
        self.Iteration, self.Residual, self.status = it.value, res.value, st
        self.ResidualNorm, self.TrueResidual, self.TrueNormalResidual = norm.value, true.value, normal.value
        if trace:
            self.trace = tr[: min(self.Iteration + 1, cap)].copy()
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            raise ApplicationException(f"LSQR did not converge within MaxIteration={self.MaxIteration}")
        if st != _lib.OK:
            check("MgcgSolveLsqr")
            raise MgcgError(f"MgcgSolveLsqr failed with status {st}")

    def Read(self):
        self.vectorX.CopyTo(self.x, self.Columns)

    def ReadResidual(self) -> np.ndarray:
        """b - A x of the last Solve()'s first closing product (rows entries)."""
        return self.vectorU.to_numpy(self.Rows)

    def ReadNormalResidual(self) -> np.ndarray:
        """A^T (b - A x) - damp^2 x of the last Solve()'s second closing product (columns entries)."""
        return self.vectorT.to_numpy(self.Columns)

    def transpose_arrays(self):
        """(elements, column_indices, row_offsets) of A^T as ``Initialize()`` formed it on the device."""
        if not self._ready:
            raise MgcgError("LeastSquaresGpu.transpose_arrays: Initialize() has not run")
        n = max(self._nnz, 1)
        return self.vectorAT.to_numpy(n)[: self._nnz], self.vectorColumnIndecesT.to_numpy(n)[: self._nnz], self.vectorRowOffsetsT.to_numpy(self.Columns + 1)
