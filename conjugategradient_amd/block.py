"""Block CG: k (1..8) right-hand sides on one matrix, every iteration reading the matrix once for all k (SolveBlockEx), and the
block product y = A x for k columns (CsrMVBlock).  The k recurrences are independent: column j is exactly the classical CG that
``ConjugateGradientSingleGpu`` runs on b[j] -- the columns share the matrix pass, nothing else.

One rank, no preconditioner, plain CSR (the handle's compression mode does not apply).  Like solver.py this module holds no
arithmetic: every flop happens in the HIP library.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .solver import ApplicationException, ConjugateGradientGpu, SparseMatrix, VectorDouble, VectorInt, _ptr


def check_block(a, k: int, count: int, name: str) -> np.ndarray:
    """a as a contiguous float64 (k, count) copy, or ValueError."""
    a = np.array(a, dtype=np.float64, order="C", copy=True)
    if a.shape != (k, count):
        raise ValueError(f"{name} has shape {a.shape}, expected (k, count) = {(k, count)}")
    return a


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _lib.BLOCK_MAX_K:
        raise ValueError(f"k = {k!r}: a block holds 1 .. {_lib.BLOCK_MAX_K} right-hand sides")
    return int(k)


class ConjugateGradientBlockGpu(ConjugateGradientGpu):
    """k independent CG solves with one matrix pass per iteration.  ``X`` and ``B`` are (k, count) arrays (row j = column j of the
    block); after ``Solve`` the attributes ``Iteration``, ``Residual`` and ``Status`` are length-k arrays and, with ``trace=True``,
    ``trace`` is a list of k per-column residual traces.  ``rule`` is one of the library's stop rules (default RULE_NATIVE)."""

    DEVICE_ID = 0

    def __init__(self, count, maxNonZeroCount, k, _minIteration, _maxIteration, allowableResidual, rule=None):
        k = _check_k(k)
        if int(count) < 1:
            raise ValueError(f"count = {count!r}: at least one row")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual)
        self.k = k
        self.rule = _lib.RULE_NATIVE if rule is None else int(rule)
        self.X = np.zeros((k, self.Count), dtype=np.float64)
        self.B = np.zeros((k, self.Count), dtype=np.float64)
        self.Iteration = np.zeros(k, dtype=np.int32)
        self.Residual = np.zeros(k, dtype=np.float64)
        self.Status = np.zeros(k, dtype=np.int32)
        self.trace = None
        self.cublas = None
        _lib.require_gpu()
        self.cublas = self.CreateBlas()
        self.cusparse = self.CreateSparse()
        self.matDescr = self.CreateMatDescr()
        n = self.Count
        self.vectorA = VectorDouble(n * maxNonZeroCount)
        self.vectorColumnIndeces = VectorInt(n * maxNonZeroCount)
        self.vectorRowOffsets = VectorInt(n + 1)
        self.vectorX = VectorDouble(k * n)
        self.vectorB = VectorDouble(k * n)
        self.vectorAp = VectorDouble(k * n)
        self.vectorP = VectorDouble(k * n)
        self.vectorR = VectorDouble(k * n)

    def Dispose(self):
        for name in ("vectorA", "vectorColumnIndeces", "vectorRowOffsets", "vectorX", "vectorB", "vectorAp", "vectorP", "vectorR"):
            v = getattr(self, name, None)
            if v is not None:
                v.Dispose()
        if self.cublas:
            lib().DestroyBlas(self.cublas)
            lib().DestroySparse(self.cusparse)
            lib().DestroyMatDescr(self.matDescr)
            self.cublas = None

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass

    def load(self, system, B, X=None):
        """A from a problems.LinearSystem; B (and the start vectors X, default the system's x in every column) as (k, count) arrays."""
        self.A = SparseMatrix.from_system(system)
        self.B = self._block(B, "B")
        self.X = np.tile(np.asarray(system.x, dtype=np.float64), (self.k, 1)) if X is None else self._block(X, "X")
        return self

    def _block(self, a, name):
        return check_block(a, self.k, self.Count, name)

    def Initialize(self):
        self.B = self._block(self.B, "B")
        self.X = self._block(self.X, "X")
        nonzeroCount = int(self.A.RowOffsets[self.Count])
        self.vectorA.CopyFrom(self.A.Elements, nonzeroCount)
        self.vectorColumnIndeces.CopyFrom(self.A.ColumnIndeces, nonzeroCount)
        self.vectorRowOffsets.CopyFrom(self.A.RowOffsets, self.Count + 1)
        self.vectorB.CopyFrom(self.B.reshape(-1), self.k * self.Count)
        self.vectorX.CopyFrom(self.X.reshape(-1), self.k * self.Count)

    def Solve(self, trace: bool = False):
        k, n = self.k, self.Count
        nonzeroCount = int(self.A.RowOffsets[n])
        it = np.zeros(k, dtype=np.int32)
        res = np.zeros(k, dtype=np.float64)
        status = np.zeros(k, dtype=np.int32)
        cap = max(self.MaxIteration, self.MinIteration) + 8 if trace else 0
        tr = np.zeros(max(k * cap, 1)) if trace else None
        L = lib()
        st = L.SolveBlockEx(self.cublas, self.cusparse, self.matDescr,
                            self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                            self.vectorX.Ptr, self.vectorB.Ptr, self.vectorAp.Ptr, self.vectorP.Ptr, self.vectorR.Ptr,
                            nonzeroCount, n, k,
                            self.AllowableResidual, self.MinIteration, self.MaxIteration, self.rule,
                            _ptr(it), _ptr(res), _ptr(status), _ptr(tr) if trace else None, cap)
        if st == _lib.ERROR:
            check("SolveBlockEx")
            raise MgcgError("SolveBlockEx failed")
        self.Iteration, self.Residual, self.Status = it, res, status
        if trace:
            self.trace = [tr[j * cap: j * cap + int(it[j]) + 1].copy() for j in range(k)]
        if st == _lib.NONFINITE:
            check("SolveBlockEx")
            raise MgcgError("SolveBlockEx: the residual of a column is not finite")
        if st == _lib.MAXIT_EXCEEDED:
            L.MgcgClearLastError()
            bad = [j for j in range(k) if status[j] == _lib.MAXIT_EXCEEDED]
            raise ApplicationException(f"CG did not converge within MaxIteration={self.MaxIteration} in columns {bad}")

    def Read(self):
        out = np.empty(self.k * self.Count)
        self.vectorX.CopyTo(out, self.k * self.Count)
        self.X = out.reshape(self.k, self.Count)


def CsrMVBlock(sparse, y_ptr: int, elements_ptr: int, row_offsets_ptr: int, column_indeces_ptr: int, x_ptr: int,
               elementsCount: int, count: int, k: int, descr=None):
    """y = A x for k columns on raw device pointers (column j of x and y at [j*count, (j+1)*count)); the C export, checked."""
    k = _check_k(k)
    if int(count) < 0 or int(elementsCount) < 0:
        raise ValueError("negative size")
    lib().CsrMVBlock(sparse, descr, y_ptr, elements_ptr, row_offsets_ptr, column_indeces_ptr, x_ptr, int(elementsCount), int(count), k)
    check("CsrMVBlock")
