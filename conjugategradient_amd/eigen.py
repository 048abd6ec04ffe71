"""LOBPCG (``MgcgSolveLobpcg``, ``MgcgSolveLobpcgMg``): the k = 1 .. 8 lowest (or highest) eigenpairs of a symmetric CSR matrix.

Every other solver of this package solves a linear system; ``MgcgEstimateSpectrum`` returns Ritz values of an unpreconditioned Lanczos run
and no vectors.  LOBPCG (Knyazev's locally optimal block preconditioned CG) returns eigenvalues, eigenvectors and their residuals, and it
takes the preconditioners the package has: none, the diagonal (``jacobi=True``) or, through ``SolveLobpcg`` of the multigrid, aggregation,
SSOR and ILU(0) classes, the cycle of their hierarchy.  include/MgcgGpu.h states the method as computed.

``SymmetricEigenGpu`` keeps A on the device.  ``Solve()`` stores ``Theta`` (k values, ascending; descending with ``largest``), ``X`` (count x
k, orthonormal columns), ``Residual`` (|| A x_j - theta_j x_j ||_2 as the loop judged it), ``TrueResidual`` (the same from one closing
product), ``Iteration`` (the last body that was judged), ``Restarts`` (how often the dense problem dropped P), ``status`` (the call's; ``ColumnStatus``: one per column)
and ``trace`` (bodies x k).  One rank.  No arithmetic happens in this module but the start block.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MgcgError, lib
from .jacobi import jacobi_setup
from .solver import ConjugateGradientSingleGpu, SparseMatrix, VectorDouble, _ptr

MAX_K = 8


def start_block(count: int, k: int, seed: int = 1) -> np.ndarray:
    """The default start block: count x k standard normal numbers, a fixed function of ``seed`` (column j is drawn after column j - 1)."""
    return np.ascontiguousarray(np.random.default_rng(int(seed)).standard_normal((int(k), int(count))).T)


def lobpcg_call(obj, export, k, head, dinv, largest, relative, trace, X0, seed, traceCapacity=None):
    """One LOBPCG solve in one native call for an object with the single-GPU classes' members (the matrix on the device, ``Count``,
    the stop members).  Stores every output on ``obj``, THEN raises ApplicationException past MaxIteration and MgcgError for every
    other status but MGCG_OK."""
    k, n = int(k), obj.Count
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{export}: k = {k} eigenpairs, must be 1 .. {MAX_K}")
    X0 = start_block(n, k, seed) if X0 is None else np.asarray(X0, dtype=np.float64)
    if X0.shape != (n, k):
        raise ValueError(f"{export}: the start block is {X0.shape}, not ({n}, {k})")
    L = lib()
    need = int(L.MgcgLobpcgWorkSize(n, k))
    if need < 1:
        raise ValueError(f"{export}: MgcgLobpcgWorkSize({n}, {k}) gives no size")
    if getattr(obj, "vectorEigenX", None) is None or obj.vectorEigenX.size < n * k:
        obj._dispose_vectors("vectorEigenX")
        obj.vectorEigenX = VectorDouble(n * k)
    if getattr(obj, "vectorEigenWork", None) is None or obj.vectorEigenWork.size < need:
        obj._dispose_vectors("vectorEigenWork")
        obj.vectorEigenWork = VectorDouble(need)
    obj.vectorEigenX.CopyFrom(np.ascontiguousarray(X0.T).reshape(-1), n * k)
    nnz = int(obj.A.RowOffsets[n]) if getattr(obj, "A", None) is not None else obj._nnz
    it, restarts = C.c_int(0), C.c_int(0)
    theta, res, true = (np.full(k, np.nan) for _ in range(3))
    status = np.zeros(k, dtype=np.int32)
    cap = (max(obj.MaxIteration, obj.MinIteration) + 8 if traceCapacity is None else int(traceCapacity)) if trace else 0
    tr = np.zeros(max(cap, 1) * k) if trace else None
    st = getattr(L, export)(obj.cublas, obj.cusparse, obj.matDescr, *head,
                            obj.vectorA.Ptr, obj.vectorRowOffsets.Ptr, obj.vectorColumnIndeces.Ptr,
                            obj.vectorEigenX.Ptr, obj.vectorEigenWork.Ptr, *dinv,
                            nnz, n, k, 1 if largest else 0,
                            obj.AllowableResidual, 1 if relative else 0, obj.MinIteration, obj.MaxIteration,
                            C.byref(it), _ptr(theta), _ptr(res), _ptr(true), _ptr(status), C.byref(restarts), _ptr(tr) if trace else None, cap)
    obj.Iteration, obj.Restarts, obj.status, obj.ColumnStatus = it.value, restarts.value, st, status.copy()
    obj.Theta, obj.Residual, obj.TrueResidual = theta, res, true
    obj.X = None
    if trace:
        rows = 0 if st == _lib.ERROR else min(obj.Iteration + 1, cap)
        obj.trace = np.ascontiguousarray(tr.reshape(k, max(cap, 1))[:, :rows].T)
    if st == _lib.ERROR:
        obj._raise_for_status(export, "LOBPCG", st)
    # X is read through a vector copy, which looks at the thread's last error too: the solve's message is set aside for it and put back,
    # so that the status is handled where every native solve's is (ConjugateGradientGpu._raise_for_status)
    message = _lib.last_error()
    L.MgcgClearLastError()
    obj.X = np.ascontiguousarray(obj.vectorEigenX.to_numpy(n * k)[: n * k].reshape(k, n).T)
    if st == _lib.MAXIT_EXCEEDED:
        obj._raise_for_status(export, "LOBPCG", st)
    if st != _lib.OK:
        raise MgcgError(f"{export}: {message}" if message else f"{export} failed with status {st}")


class SymmetricEigenGpu(ConjugateGradientSingleGpu):
    """The k extreme eigenpairs of the symmetric matrix ``A`` (count rows, at most ``maxNonzero`` stored entries per row): ``load(system)``,
    ``Initialize()``, ``Solve(trace=False, X0=None, seed=1)``, ``Read()`` (returns ``Theta``, ``X``).  ``relative``: a column is converged when
    its residual norm is at most allowableResidual |theta_j| (else: at most allowableResidual); ``jacobi``: precondition with diag(A)^-1."""

    def __init__(self, count, maxNonzero, k, minIteration, maxIteration, allowableResidual, relative=True, largest=False, jacobi=False):
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"SymmetricEigenGpu: k = {k} eigenpairs, must be 1 .. {MAX_K}")
        if 3 * int(k) > int(count):
            raise ValueError(f"SymmetricEigenGpu: k = {k} eigenpairs need 3 k <= count = {count}")
        super().__init__(count, maxNonzero, minIteration, maxIteration, allowableResidual, rule=_lib.RULE_CSHARP)
        self.k, self.relative, self.largest, self.jacobi = int(k), bool(relative), bool(largest), bool(jacobi)
        self.vectorDinv = VectorDouble(count) if jacobi else None
        self.vectorEigenX = self.vectorEigenWork = None
        self.Theta = self.X = self.TrueResidual = None
        self.Restarts, self._ready = 0, False

    def Dispose(self):
        self._dispose_vectors("vectorDinv", "vectorEigenX", "vectorEigenWork")
        super().Dispose()

    def load(self, system):
        """Take A from a ``problems.LinearSystem`` (or anything with its CSR members); its x and b are not used."""
        self.A = SparseMatrix.from_system(system)
        return self

    def Initialize(self):
        self._ready = False
        super().Initialize()
        if self.jacobi:
            jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces, int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def Solve(self, trace: bool = False, X0=None, seed: int = 1, traceCapacity=None):
        if not self._ready:
            raise MgcgError("SymmetricEigenGpu.Solve: Initialize() has not run")
        lobpcg_call(self, "MgcgSolveLobpcg", self.k, (), (self.vectorDinv.Ptr if self.jacobi else None,), self.largest, self.relative, trace, X0, seed, traceCapacity)

    def Read(self):
        return self.Theta, self.X
