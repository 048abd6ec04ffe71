"""Multicolour ILU(0)-preconditioned CG, MINRES, BiCGStab and GMRES(m) for any CSR matrix with a structurally symmetric pattern.

The preconditioner is ``MgSetupIlu0``: the incomplete factorisation without fill of A + shift * diag(A) in the colour order of the
multicolour Gauss-Seidel smoother (include/MgcgGpu.h writes the contract out; tests/test_ilu_host.py states it in numpy), M^-1 = U^-1 L^-1
as one forward and one backward pass over a factor whose colours are contiguous.  What a matrix with no grid and no negative couplings to
coarsen gets beyond the diagonal (``jacobi``) and SSOR (``ssor``).  The CG and MINRES forms need a symmetric A and positive pivots
(``pivot_range()``; ``shift > 0`` is the usual remedy); BiCGStab and GMRES(m) ask nothing of M.  ``Apply``, ``Solve``, ``SolveMinres``,
``SolveBicgstab`` and ``SolveGmres`` are the parent's, ``hierarchy=`` included; no arithmetic on vectors happens here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MgcgError, check, lib
from .amg import ConjugateGradientAmgGpu
from .solver import _ptr


class ConjugateGradientIluGpu(ConjugateGradientAmgGpu):
    """ConjugateGradientAmgGpu whose ``mg`` is an ILU(0) factor (one level); ``shift`` >= 0 factors A + shift * diag(A)."""

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, shift: float = 0.0, rule=_lib.RULE_CSHARP):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, levels=1, aggregates=[], rule=rule)
        self.shift = float(shift)

    def Setup(self):
        nonzeroCount = int(self.A.RowOffsets[self.Count]) if self.A is not None else self._nnz
        L = lib()
        if self.mg:
            L.MgDestroy(self.mg)
            self.mg = None
        self.mg = L.MgSetupIlu0(self.cublas, self.cusparse, self.vectorA.Ptr, self.vectorRowOffsets.Ptr, self.vectorColumnIndeces.Ptr,
                                nonzeroCount, self.Count, self.shift)
        check("MgSetupIlu0")
        if not self.mg:
            raise MgcgError("MgSetupIlu0 returned NULL")
        self.levels = L.MgLevels(self.mg)

    def colours(self) -> int:
        """The colours of the order."""
        c = lib().MgIluColours(self.mg)
        check("MgIluColours")
        return c

    def pivot_range(self):
        """(smallest, largest) pivot of the factor; the CG and MINRES forms need both positive."""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        if lib().MgIluPivotRange(self.mg, C.byref(lo), C.byref(hi)) != 0:
            check("MgIluPivotRange")
            raise MgcgError("MgIluPivotRange failed")
        return lo.value, hi.value

    def setup_ms(self):
        """Milliseconds the last ``Setup()`` took on the host's clock: (checks and colouring, building B, factorisation)."""
        ms = np.zeros(3)
        if lib().MgIluSetupMs(self.mg, _ptr(ms)) != 0:
            check("MgIluSetupMs")
            raise MgcgError("MgIluSetupMs failed")
        return tuple(float(v) for v in ms)

    def factor(self):
        """(elements, columnIndeces, rowOffsets, diagonal, rowOf): the factor of B = P (A + shift diag(A)) P^T as CSR in the new order with
        sorted rows (L's multipliers left of every row's diagonal, U from the pivot on), the position of every row's diagonal, and
        ``rowOf[new] = old``."""
        L = lib()
        nnz = L.MgIluCopyFactor(self.mg, None, None, None, None, None)
        if nnz < 0:
            check("MgIluCopyFactor")
            raise MgcgError("MgIluCopyFactor failed")
        n = self.Count
        e, c, ro = np.empty(nnz), np.empty(nnz, dtype=np.int32), np.empty(n + 1, dtype=np.int32)
        d, rowOf = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        if L.MgIluCopyFactor(self.mg, _ptr(e), _ptr(c), _ptr(ro), _ptr(d), _ptr(rowOf)) != nnz:
            check("MgIluCopyFactor")
            raise MgcgError("MgIluCopyFactor failed")
        return e, c, ro, d, rowOf
