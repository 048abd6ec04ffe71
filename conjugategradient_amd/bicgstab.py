"""BiCGStab and BiCGStab(l) (``SolveBicgstab``, ``SolveBicgstabJacobi``, ``SolveBicgstabL``, ``SolveBicgstabLJacobi``): nonsymmetric systems
A x = b.

Every other loop of this package takes a symmetric matrix: on a convection-diffusion stencil, an upwinded operator or any CSR matrix with
A != A^T the CG loops break down or return a wrong x, and MINRES is not defined.  BiCGStab (van der Vorst) needs only products with A --
no transpose, no new matrix form -- and fixed storage: two products and three global sums per iteration.  It is right-preconditioned, so
the residual it carries is that of the system itself and every stop rule judges its 2-norm, as everywhere else here.

``BiConjugateGradientStabGpu`` has ``MinimalResidualGpu``'s class surface.  ``Iteration``, ``Residual`` and the trace show the
recurrence's residual, which can drift from b - A x on a badly conditioned nonsymmetric matrix; ``TrueResidual`` is || b - A x ||_2 from
one closing product, and ``ReadResidual()`` returns that vector.  ``BiConjugateGradientStabJacobiGpu`` is the same class with M = diag(A).
Several ranks: ``ConjugateGradientRankGpu.SolveBicgstab`` / ``.SolveBicgstabJacobi``.  The V-cycle as right preconditioner
(``SolveBicgstabMg``) is the method ``SolveBicgstab(trace=False, hierarchy=None)`` of ``multigrid.ConjugateGradientMgGpu`` and
``amg.ConjugateGradientAmgGpu``: the hierarchy is the object's own, built from the nonsymmetric matrix itself, or with ``hierarchy`` that
of another multigrid object -- one built from ``problems.symmetric_part(system)``, say.

BiCGStab's residual polynomial has real roots only -- one minimal-residual step of degree 1 per body -- and where convection dominates (a
spectrum near the imaginary axis) it stagnates or breaks down.  ``BiConjugateGradientStabLGpu(..., ell=2)`` is BiCGStab(l) (Sleijpen and
Fokkema, ``SolveBicgstabL``): a body is ``ell`` BiCG steps and one minimal-residual step of degree ``ell``, 1 <= ell <= 4, so ``Iteration``,
``MinIteration``, ``MaxIteration`` and the trace count bodies of ``2 * ell`` products.  Same surface as ``BiConjugateGradientStabGpu``;
``BiConjugateGradientStabLJacobiGpu`` is the same with M = diag(A).  One rank; no V-cycle form yet.

The max-norm stop rule is not supported by any of them.  No arithmetic happens in this module.
"""
from __future__ import annotations

from . import _lib
from ._lib import MgcgError
from .jacobi import check_system_shapes, jacobi_setup
from .solver import ConjugateGradientSingleGpu, VectorDouble

_WORK = ("vectorV", "vectorS", "vectorT", "vectorRhat")


class BiConjugateGradientStabGpu(ConjugateGradientSingleGpu):
    """ConjugateGradientSingleGpu on the BiCGStab loop: same constructor, members, ``Iteration`` / ``Residual`` and
    ``ApplicationException`` behaviour, for any CSR matrix.  ``ReadResidual()`` returns the true residual b - A x that the last Solve()'s
    closing product left in its work vector."""

    _export = "SolveBicgstab"
    _what = "BiCGStab"
    _work_names = _WORK                # the work vectors of `count` entries that the constructor allocates
    _jacobi = False                    # with M = diag(A): ``vectorDinv``, filled and checked by Initialize(), follows the work vectors

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None):
        if rule == _lib.RULE_HANDMADECL:
            raise ValueError(f"{type(self).__name__}: the max-norm rule (RULE_HANDMADECL) is not supported")
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.TrueResidual = float("nan")
        for name in self._work_names + (("vectorDinv",) if self._jacobi else ()):
            setattr(self, name, VectorDouble(count))
        self._ready = False

    def Dispose(self):
        self._dispose_vectors(*_WORK, "vectorDinv", "vectorWork")
        self._work_size = 0
        super().Dispose()

    def Initialize(self):
        self._ready = False
        check_system_shapes(self.A, self.x, self.b, self.Count)
        super().Initialize()
        if self._jacobi:
            jacobi_setup(self.cusparse, self.vectorA, self.vectorRowOffsets, self.vectorColumnIndeces,
                         int(self.A.RowOffsets[self.Count]), self.Count, 0, self.vectorDinv)
        self._ready = True

    def _more_vectors(self):
        return (self.vectorDinv.Ptr,) if self._jacobi else ()

    def _work_arguments(self):
        """What the export takes between the r vector and the sizes."""
        return (self.vectorV.Ptr, self.vectorS.Ptr, self.vectorT.Ptr, self.vectorRhat.Ptr, *self._more_vectors())

    def Solve(self, trace: bool = False, traceCapacity: int | None = None):
        """trace: keep the residual trace in ``self.trace``; traceCapacity: its length when the default (room for every iteration) is not wanted."""
        if not self._ready:
            raise MgcgError(f"{type(self).__name__}.Solve: Initialize() has not run")
        self._native_solve(self._export, self._what, trace, work=self._work_arguments(), third=("TrueResidual", float("nan")),
                           traceCapacity=traceCapacity)


class BiConjugateGradientStabJacobiGpu(BiConjugateGradientStabGpu):
    """BiConjugateGradientStabGpu with M = diag(A) as right preconditioner (SolveBicgstabJacobi): same constructor and members, and the
    same residual -- that of A x = b in the 2-norm.  ``Initialize()`` also extracts and checks the diagonal (a row without a positive,
    finite stored diagonal raises ``MgcgError`` there)."""

    _export = "SolveBicgstabJacobi"
    _what = "Jacobi-preconditioned BiCGStab"
    _jacobi = True


class OneWorkVectorGpu(BiConjugateGradientStabGpu):
    """BiConjugateGradientStabGpu for the loops that keep their vectors in one work vector (BiCGStab(l), GMRES(m)): ``vectorWork`` of
    ``_slices()`` slices replaces v, s, t and rhat.  It is sized by the constructor and allocated again, larger, by the first ``Solve()``
    after the object's sizes were raised."""

    _work_names = ()
    _slices_more = property(lambda self: 1 if self._jacobi else 0)     # the diagonal's form keeps one slice more

    def _slices(self):
        """How many slices the loop needs now (for a size the library refuses: as for the nearest it takes, so that the call reaches
        its refusal)."""
        raise NotImplementedError


class BiConjugateGradientStabLGpu(OneWorkVectorGpu):
    """BiConjugateGradientStabGpu on the BiCGStab(l) loop (SolveBicgstabL): same members, ``TrueResidual``, ``ReadResidual()``, trace and
    exceptions; ``ell`` (1 .. 4) is the degree of a body's minimal-residual step, and iterations count bodies of ``2 * ell`` products.  One
    work vector of ``2 * ell`` slices (one more with the diagonal) replaces v, s, t and rhat: it is sized for the object's ``ell`` and
    allocated again, larger, by the first ``Solve()`` after ``ell`` was raised.  The library checks ``ell`` and the vector's size; an
    ``ell`` it refuses leaves the object usable with another."""

    _export = "SolveBicgstabL"
    _what = "BiCGStab(l)"

    def __init__(self, count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=None, ell=2):
        super().__init__(count, maxNonZeroCount, _minIteration, _maxIteration, allowableResidual, rule=rule)
        self.ell = int(ell)
        self._ensure_work(self._slices())

    def _slices(self):
        return 2 * min(max(int(self.ell), 1), 4) + self._slices_more

    def _work_arguments(self):
        self._ensure_work(self._slices())
        return (self.vectorWork.Ptr, *self._more_vectors(), int(self.ell))


class BiConjugateGradientStabLJacobiGpu(BiConjugateGradientStabLGpu):
    """BiConjugateGradientStabLGpu with M = diag(A) as right preconditioner (SolveBicgstabLJacobi); ``Initialize()`` also extracts and
    checks the diagonal, as ``BiConjugateGradientStabJacobiGpu`` does."""

    _export = "SolveBicgstabLJacobi"
    _what = "Jacobi-preconditioned BiCGStab(l)"
    _jacobi = True
