"""Multigrid-preconditioned CG ("MGCG") on one GPU through the C ABI (MgSetup / MgApply / SolveMg).

The reference names itself MGCG (Mgcg/cuBlas/Mgcg/MgcgMain.cs:8) but never implemented the
preconditioner; DESIGN.md section 6 defines the one built here (cell-centred geometric hierarchy,
piecewise-constant transfer, Galerkin coarse operators scaled by 1/2, weighted-Jacobi V(nu,nu)).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .bicgstab import _WORK as _BICGSTAB_WORK          # vectorV, vectorS, vectorT, vectorRhat
from .gmres import MAX_M as _GMRES_MAX_M
from .solver import ConjugateGradientSingleGpu, VectorDouble, _ptr

_TRUE = ("TrueResidual", float("nan"))                 # the third output of SolveMinres, SolveBicgstab and SolveGmres


class ConjugateGradientMgGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu plus a V-cycle preconditioner built from ``grid = (nx, ny, nz)``.  ``ReadResidual()`` returns the true
    residual that the closing product of the last SolveMinres(), SolveBicgstab() or SolveGmres() left in its work vector."""

    _default_rule = _lib.RULE_CSHARP        # what rule=None means here (the one-rank classes without a hierarchy: RULE_NATIVE)

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, grid,
                 levels: int = 3, omega: float | None = None, nu: int = 1, nuCoarse: int = 4, sigma: float = 0.5,
                 rule=_lib.RULE_CSHARP, interpolation: int = 0):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.interpolation = int(interpolation)          # 0: piecewise constant, 1: cell-centred linear (MgSetInterpolation)
        self.grid = tuple(int(g) for g in grid)
        nx, ny, nz = self.grid
        if nx * ny * nz != count:
            raise MgcgError("grid does not match count")
        self.levels_requested = levels
        self.omega = (6.0 / 7.0 if nz > 1 else 4.0 / 5.0) if omega is None else float(omega)
        self.nu, self.nuCoarse, self.sigma = int(nu), int(nuCoarse), float(sigma)
        self.vectorZ = VectorDouble(count)
        self.mg = None

    def Dispose(self):
        if getattr(self, "mg", None):
            lib().MgDestroy(self.mg)
            self.mg = None
        # with SolveMinres's, SolveGmres's and SolveBicgstab's work space, if they ran
        self._dispose_vectors("vectorZ", "vectorW1", "vectorW2", "vectorR1", "vectorWork", "vectorEigenX", "vectorEigenWork", *_BICGSTAB_WORK)
        self._work_size = 0
        super().Dispose()

    def Initialize(self):
        super().Initialize()
        self.Setup()

    def InitializePoisson(self, b_value: float = 1.0, x_value: float = 0.0):
        """Generate the 5/7-point Poisson matrix of ``self.grid`` directly in HBM (no host arrays) and build
        the hierarchy; the 512^3 system is 11.8 GB and is never materialised on the host."""
        L = lib()
        nx, ny, nz = self.grid
        nnz = L.MgcgPoissonNnz(nx, ny, nz, 0, nz)
        if self.vectorA.size < nnz:
            raise MgcgError("construct with maxNonZeroCount >= 7 for the Poisson generator")
        if L.MgcgGeneratePoisson(self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr, nx, ny, nz, 0, nz) != 0:
            check("MgcgGeneratePoisson")
        L.MgcgFill(self.vectorB.Ptr, b_value)
        L.MgcgFill(self.vectorX.Ptr, x_value)
        self.A = None
        self._nnz = int(nnz)
        self.Setup()

    def Setup(self):
        nx, ny, nz = self.grid
        nonzeroCount = int(self.A.RowOffsets[self.Count]) if self.A is not None else self._nnz
        if self.mg:
            lib().MgDestroy(self.mg)
        self.mg = lib().MgSetup(self.cublas, self.cusparse, self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                                nonzeroCount, nx, ny, nz, self.levels_requested, self.omega, self.nu, self.nuCoarse, self.sigma)
        check("MgSetup")
        if not self.mg:
            raise MgcgError("MgSetup returned NULL")
        if self.interpolation and lib().MgSetInterpolation(self.mg, self.interpolation) != 0:
            check("MgSetInterpolation")
        self.levels = lib().MgLevels(self.mg)

    def level_csr(self, l: int):
        n, nnz = lib().MgLevelRows(self.mg, l), lib().MgLevelNnz(self.mg, l)
        e, c, r = np.empty(nnz), np.empty(nnz, dtype=np.int32), np.empty(n + 1, dtype=np.int32)
        lib().MgLevelCopyCsr(self.mg, l, _ptr(e), _ptr(c), _ptr(r))
        check("MgLevelCopyCsr")
        return e, c, r

    def level_dinv(self, l: int):
        d = np.empty(lib().MgLevelRows(self.mg, l))
        lib().MgLevelCopyDinv(self.mg, l, _ptr(d))
        check("MgLevelCopyDinv")
        return d

    def Apply(self, r: np.ndarray) -> np.ndarray:
        """z = M^-1 r for a host vector (test helper)."""
        vr, vz = VectorDouble(self.Count), VectorDouble(self.Count)
        vr.CopyFrom(np.ascontiguousarray(r, dtype=np.float64), self.Count)
        lib().MgApply(self.mg, vr.ToRawPtr(), vz.ToRawPtr())
        check("MgApply")
        z = vz.to_numpy()
        vr.Dispose()
        vz.Dispose()
        return z

    def Solve(self, trace: bool = False):
        self._native_solve("SolveMg", "MGCG", trace, head=(self.mg,), work=(self.vectorZ.Ptr,))

    def SolveMinres(self, shift: float = 0.0, trace: bool = False):
        """Solve (A - shift I) x = b with MINRES preconditioned by this hierarchy's V-cycle (SolveMinresMg): A symmetric, definite or not.
        The hierarchy is ``self.mg`` whatever matrix it was built from (only its row count is checked); ``w1``, ``w2`` and ``r1`` are
        allocated at the first call.  ``Iteration``, ``Residual`` and ``trace`` show the residual in the M^-1 norm, sqrt(r . M^-1 r),
        which is what the stop rule judges; ``TrueResidual`` is the plain 2-norm || b - (A - shift I) x ||_2 of the closing product, and
        ``vectorR`` holds that vector."""
        self._ensure_vectors(self.Count, "vectorW1", "vectorW2", "vectorR1")      # (Count is fixed: one that exists is never too small)
        self._native_solve("SolveMinresMg", "V-cycle-preconditioned MINRES", trace, head=(self.mg,), more=(float(shift),),
                           work=(self.vectorR1.Ptr, self.vectorW1.Ptr, self.vectorW2.Ptr, self.vectorZ.Ptr), third=_TRUE)

    def SolveBicgstab(self, trace: bool = False, hierarchy=None):
        """Solve A x = b, A any CSR matrix, with BiCGStab right-preconditioned by a hierarchy's V-cycle (SolveBicgstabMg).  The
        hierarchy is ``self.mg``, built from the matrix itself -- right-preconditioned BiCGStab asks nothing of M but a fixed linear map --
        or, with ``hierarchy``, the ``mg`` of another multigrid object with as many rows, which stays that object's (the supported way to
        precondition with the hierarchy of another matrix, ``problems.symmetric_part(system)`` for instance).  ``vectorV``, ``vectorS``,
        ``vectorT`` and ``vectorRhat`` are allocated at the first call.  ``Iteration``, ``Residual`` and ``trace`` show the recurrence's
        2-norm residual; ``TrueResidual`` is || b - A x ||_2 of the closing product and ``ReadResidual()`` returns that vector."""
        self._ensure_vectors(self.Count, *_BICGSTAB_WORK)
        self._native_solve("SolveBicgstabMg", "V-cycle-preconditioned BiCGStab", trace, head=(self.mg if hierarchy is None else hierarchy.mg,),
                           work=(self.vectorV.Ptr, self.vectorS.Ptr, self.vectorT.Ptr, self.vectorRhat.Ptr), third=_TRUE)

    def SolveLobpcg(self, k: int, trace: bool = False, hierarchy=None, relative: bool = True, X0=None, seed: int = 1):
        """The k = 1 .. 8 lowest eigenpairs of the symmetric matrix A by LOBPCG preconditioned with a hierarchy's cycle (MgcgSolveLobpcgMg;
        ``eigen`` has the results' members: ``Theta``, ``X``, ``Residual``, ``TrueResidual``, ``Iteration``, ``Restarts``, ``status``,
        ``ColumnStatus``, ``trace``).  The hierarchy is ``self.mg`` or, with ``hierarchy``, the ``mg`` of another object with as many rows;
        b and x take no part.  ``AllowableResidual`` bounds || A x_j - theta_j x_j ||_2, relative to |theta_j| unless ``relative`` is false."""
        from .eigen import lobpcg_call
        lobpcg_call(self, "MgcgSolveLobpcgMg", k, (self.mg if hierarchy is None else hierarchy.mg,), (), False, relative, trace, X0, seed)

    def SolveGmres(self, trace: bool = False, hierarchy=None, m: int = 20, orth: int = 2):
        """Solve A x = b, A any CSR matrix, with restarted GMRES(m) right-preconditioned by a hierarchy's V-cycle in the flexible form
        (SolveGmresMg): the loop for the systems on which ``SolveBicgstab`` ends MGCG_NONFINITE -- where it converges, ``SolveBicgstab``
        is the faster one.  The hierarchy is ``self.mg`` or, with ``hierarchy``, the ``mg`` of another multigrid object with as many
        rows, as in ``SolveBicgstab``.  ``m`` (1 .. 32) is the restart length, ``orth`` (1 or 2) the number of classical Gram-Schmidt
        passes per step; the library checks both.  ``vectorWork`` holds the ``2 m + 1`` slices v_0 .. v_m, z_0 .. z_{m-1}: it is
        allocated at the first call and again, larger, when ``m`` has grown.  ``Iteration``, ``Residual`` and ``trace`` count Arnoldi
        steps (one cycle and one product each) and show the rotated estimate of || b - A x ||_2; ``TrueResidual`` is that norm itself
        from the closing product and ``ReadResidual()`` returns that vector."""
        self._ensure_work(2 * min(max(int(m), 1), _GMRES_MAX_M) + 1)
        self._native_solve("SolveGmresMg", "V-cycle-preconditioned GMRES(m)", trace, head=(self.mg if hierarchy is None else hierarchy.mg,),
                           work=(self.vectorWork.Ptr, int(m), int(orth)), third=_TRUE)
