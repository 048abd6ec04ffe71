"""MI355X-native CG / MGCG hot path of aokomoriuta/ConjugateGradient behind the reference's C ABI.

``_lib``      ctypes binding of libMgcgGpu.so (include/MgcgGpu.h)
``solver``    LinerEquations / ConjugateGradient / ...SingleGpu / ...ParallelGpu (reference class surface)
``parallel``  one-process-per-GPU driver (RCCL inside the library; torch.distributed bootstrap)
``multigrid`` the V-cycle preconditioner the reference named but never wrote
``amg``       the same V-cycle for ANY CSR matrix: aggregates from the matrix graph (MgSetupAggregation) or from the caller;
              ``strength="symmetric"`` (MgSetupAggregationEx) matches on the symmetric part, for A != A^T that does not coarsen otherwise
              ``amg.csr_transpose_gpu`` / ``amg.transpose_gpu``: A^T of any CSR matrix formed on the device (MgcgCsrTranspose), values as bit copies
              ``amg.csr_multiply_gpu`` / ``amg.multiply_gpu``: C = A B of two CSR matrices formed on the device (MgcgCsrMultiply), every sum in a fixed order
``ssor``      SSOR(omega)-preconditioned CG / MINRES / BiCGStab: the one-level form of ``amg`` with two multicolour Gauss-Seidel sweeps
``ilu``       multicolour ILU(0)-preconditioned CG / MINRES / BiCGStab / GMRES(m) (MgSetupIlu0): the incomplete factorisation in the colour
              order of ``ssor``, stored so that every colour is one contiguous stream and M^-1 reads the factor once
``jacobi``    Jacobi-preconditioned CG for general CSR matrices (the call the ViennaCL front-end left commented out)
``singlereduce`` single-reduction (Chronopoulos-Gear) CG: one global sum and two launches per iteration, with or without the diagonal
``minres``   MINRES for symmetric indefinite and shifted systems (A - shift I) x = b: the solver for what the CG loops refuse,
             plain or preconditioned by the diagonal (the V-cycle form is a method of the ``multigrid`` / ``amg`` classes)
``bicgstab`` BiCGStab for NONSYMMETRIC systems A x = b (convection-diffusion, upwinded stencils, any CSR matrix), plain or
             right-preconditioned by the diagonal (the V-cycle form, SolveBicgstabMg, is the ``SolveBicgstab`` method of the
             ``multigrid`` / ``amg`` classes, with the hierarchy of the matrix itself or of another one); and BiCGStab(l), l = 1 .. 4
             (``BiConjugateGradientStabLGpu``, SolveBicgstabL), for the convection-dominated systems on which BiCGStab breaks down
``gmres``    restarted GMRES(m) for NONSYMMETRIC systems (``GeneralizedMinimalResidualGpu``, SolveGmres), plain or right-preconditioned by
             the diagonal: the residual never increases, no breakdown on a nonsingular matrix, no drift -- slower per product than ``bicgstab``
             (the V-cycle form, SolveGmresMg -- flexible GMRES -- is the ``SolveGmres`` method of the ``multigrid`` / ``amg`` / ``ssor``
             classes: it converges where SolveBicgstabMg breaks down)
``lsqr``     LSQR for least squares min || A x - b ||_2 with ANY CSR matrix (``LeastSquaresGpu``, MgcgSolveLsqr): rectangular, rank deficient
             (minimum-norm solution), inconsistent right-hand sides, Tikhonov damping; A^T is formed on the device (MgcgCsrTranspose)
``eigen``    LOBPCG for the k = 1 .. 8 lowest or highest EIGENPAIRS of a symmetric CSR matrix (``SymmetricEigenGpu``, MgcgSolveLobpcg): values,
             vectors and residuals, plain or preconditioned by the diagonal (the V-cycle form, MgcgSolveLobpcgMg, is the ``SolveLobpcg``
             method of the ``multigrid`` / ``amg`` / ``ssor`` / ``ilu`` classes)
``chebyshev`` Chebyshev-preconditioned CG: a polynomial preconditioner for any CSR matrix, m products and two global sums per iteration
``shifted``   multi-shift CG: (A + s_j I) x_j = b for up to 8 shifts from one CG recurrence on A
``blockkrylov`` shared-subspace block CG: up to 8 right-hand sides in one block Krylov space (fewer iterations than ``block``)
``mixed``     mixed-precision CG: an fp32 recurrence corrected by fp64 reliable updates, fp64-accurate x and stop test
``problems``  the linear systems the reference hard-codes + the BASELINE.json stencils
"""
__all__ = ["_lib", "solver", "parallel", "multigrid", "amg", "ssor", "ilu", "jacobi", "singlereduce", "minres", "bicgstab", "gmres", "lsqr", "eigen", "chebyshev", "shifted", "blockkrylov", "mixed", "problems"]
