// Chebyshev-preconditioned CG (SolveChebyshev / SolveChebyshevParallel) for gfx950: the vector passes around the polynomial's steps.
//
// The preconditioner is z = p_m(B) u with B = D^-1 A and u = D^-1 r (B = A, u = r without the diagonal), p_m the degree m - 1 polynomial
// that the Chebyshev iteration for B z = u from z = 0 reaches after m steps on the interval [lmin, lmax]:
//     first   d = it * u ; z = d                                                    it = 1 / theta
//     step j  d = c1_j * d + c2_j * (dinv * (r - A z)) ; z' = z + d                 j = 1 .. m - 1
// A step is ONE launch: the plain-CSR product with the EPI_CHEBYSHEV epilogue (spmv_epilogue.hpp, kernels_spmv.hip), which prefetches r_i, d_i
// and dinv_i behind the gathers, stores d_i and returns z'_i; the last step (EPI_CHEBYSHEV_DOT) adds r_i * z'_i to its workgroup's partial
// sum.  No global sum anywhere in the polynomial; the coefficients are kernel arguments.  What is here: the start, the fused first pass (the
// loop's r update, the partial sums of r.r, d and z in one pass: Ap, r, dinv in; r, d, z out), the two one-workgroup scalar kernels and the
// Gershgorin bound.  The x / p update is the preconditioned loop's update_xp_kernel (kernels_blas1.hip).
//
// Every product is rounded into a double of its own before the add that follows it.  The first pass walks its elements exactly as
// update_r_kernel does and the start as copy_dot_kernel does, so with m = 1 and theta = 1 (it = 1, d = 1 * u = u) every partial sum holds the
// bits the Jacobi-preconditioned loop's passes produce, whatever the dot order.
#include "vec_passes.hpp"

namespace mgcg {

// one element of the first pass and of the start: u = dinv * r, d = it * u, with RZ the term r * d
template <bool DINV, bool RZ>
__device__ __forceinline__ double cheb_first_term(double it, double dinv, double r, double& accZ)
{
    double u = r;
    if constexpr (DINV) u = dinv * r;
    const double dv = it * u;
    if constexpr (RZ) { double t = r * dv; accZ += t; }
    return dv;
}

// ------------------------------------------------------------------ the start: d = it * (dinv r) ; z = d ; partial r.r [, r.z]
template <bool V2, bool DINV, bool RZ>
__global__ __launch_bounds__(kBlock) void cheb_start_kernel(const double* __restrict__ r, const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z,
                                                            long long n, double it, double* __restrict__ partials, double* __restrict__ partialsZ)
{
    __shared__ double s_red[4];
    double acc = 0.0, accZ = 0.0;
    grid_stride<V2>(n,
        [&](long long i) {
            d2 rv = *(const d2*)(r + i), dv = {}, zv;
            if constexpr (DINV) dv = *(const d2*)(dinv + i);
            zv.x = cheb_first_term<DINV, RZ>(it, dv.x, rv.x, accZ); zv.y = cheb_first_term<DINV, RZ>(it, dv.y, rv.y, accZ);
            *(d2*)(d + i) = zv; *(d2*)(z + i) = zv;
            double t0 = rv.x * rv.x; double t1 = rv.y * rv.y; acc += t0; acc += t1; },
        [&](long long i) {
            double rv = r[i], dv = 0.0;
            if constexpr (DINV) dv = dinv[i];
            const double zv = cheb_first_term<DINV, RZ>(it, dv, rv, accZ);
            d[i] = zv; z[i] = zv;
            double t = rv * rv; acc += t; });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if constexpr (RZ) {
        __shared__ double s_red2[4];
        const double tz = block_sum(accZ, s_red2);
        if (threadIdx.x == 0) partialsZ[blockIdx.x] = tz;
    }
}
int launch_cheb_start(hipStream_t s, const double* r, const double* dinv, double* d, double* z, long long n, double it,
                      double* partials, double* partialsZ, bool withRz)
{
    if (n < 0) n = 0;
    const bool v2 = al16(r) && al16(dinv) && al16(d) && al16(z);
    const int grid = grid_for(n, v2 ? 4 : 2);
    with_flags([&](auto V2, auto DINV, auto RZ) {
        hipLaunchKernelGGL((cheb_start_kernel<V2.value, DINV.value, RZ.value>), dim3(grid), dim3(kBlock), 0, s, r, dinv, d, z, n, it, partials, partialsZ);
    }, v2, dinv != nullptr, withRz);
    if (dot_reference_order()) {                                      // the sums in the reference's order replace the partial sums
        launch_dot_serial(s, r, r, n, partials, nullptr);
        if (withRz) launch_dot_serial(s, r, z, n, partialsZ, nullptr);
        return 1;
    }
    return grid;
}

// What a loop that stops on a breakdown publishes, by one thread: the last judged residual once more in the trace entry of the iteration
// that could not run, the status, the host mirror (its `done` last, behind a system-wide fence).
__device__ __forceinline__ void cheb_publish_breakdown(const FinalizeArgs& f, int it, double rr, double rr0)
{
    CgScalars* sc = f.sc;
    const double res = sqrt(rr);
    const double shown = f.rule == MGCG_RULE_VIENNACL ? sqrt(rr / rr0) : res;
    if (f.trace != nullptr && it < f.traceCap) f.trace[it] = shown;
    sc->residual = res; sc->iteration = it; sc->done = 1; sc->status = MGCG_NONFINITE;
    f.mirror->residual = res; f.mirror->iteration = it; f.mirror->status = MGCG_NONFINITE;
    __threadfence_system();
    f.mirror->done = 1;
}

// ------------------------------------------------------------------ the scalars in front of iteration 0 (one workgroup)
__global__ __launch_bounds__(kBlock) void cheb_init_scalars_kernel(const double* __restrict__ partials, int n, const double* __restrict__ partialsZ, int nZ,
                                                                   int reduceFirst, FinalizeArgs f)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    CgScalars* sc = f.sc;
    double rr = 0.0, rz = 0.0;
    if (reduceFirst) {
        rr = reduce_partials_block(partials, n, s_red, 0);
        rz = reduce_partials_block(partialsZ, nZ, s_red2, 0);
    }
    if (threadIdx.x != 0) return;
    if (!reduceFirst) { rr = sc->rrNew; rz = sc->rzNew; }             // (several ranks: the all-reduced pair)
    sc->rr = rz; sc->rr0 = rr; sc->pAp = 0; sc->rrNew = rr; sc->rzNew = rz; sc->residual = 0; sc->nrmInf = 0;
    sc->beta = 0; sc->alpha = 0; sc->iteration = 0; sc->done = 0; sc->status = 0; sc->pad = 0;
    sc->fRr = rz; sc->fRr0 = rr; sc->fAlpha = 0; sc->fIteration = 0; sc->fDone = 0; sc->pSlot = 0;
    f.mirror->residual = 0; f.mirror->iteration = 0; f.mirror->status = 0; f.mirror->done = 0;
    if (!positive_finite(rz)) cheb_publish_breakdown(f, 0, rr, rr);     // an indefinite polynomial (upper bound below the spectrum), or r = 0
}
void launch_cheb_init_scalars(hipStream_t s, const double* partials, int n, const double* partialsZ, int nZ, bool reduceFirst, const FinalizeArgs& f)
{
    hipLaunchKernelGGL(cheb_init_scalars_kernel, dim3(1), dim3(kBlock), 0, s, partials, n, partialsZ, nZ, reduceFirst ? 1 : 0, f);
}

// ------------------------------------------------------------------ the fused first pass
// alpha = r.z / p.Ap ; r = r + (-alpha)*Ap ; partial r.r ; d = it * (dinv * r) ; z = d [; partial r.z: degree 1, where no step follows]
// Five streams (Ap, r in; r, d, z out), six with dinv: 40 (48) bytes per row.  One rank: every workgroup adds the p.Ap partial sums of the
// product itself, as update_r_kernel does.  A p.Ap that is not finite and > 0 ends the loop before anything is written: every workgroup
// sees the same sum and returns, the first one publishes.
template <bool V2, bool NTV, bool DINV, bool RZ>
__global__ __launch_bounds__(kBlock) void cheb_first_kernel(FinalizeArgs f, double* __restrict__ r, const double* __restrict__ Ap, const double* __restrict__ dinv,
                                                            double* __restrict__ d, double* __restrict__ z, long long n, double it,
                                                            double* __restrict__ partials, double* __restrict__ partialsZ,
                                                            const double* __restrict__ pApPartials, int nPAp)
{
    __shared__ double s_red[4];
    __shared__ double s_pAp;
    CgScalars* sc = f.sc;
    if (sc->done != 0) return;
    double pAp;
    if (pApPartials != nullptr) {
        const double t = reduce_partials_block(pApPartials, nPAp, s_red, 0);
        if (threadIdx.x == 0) s_pAp = t;
        __syncthreads();
        pAp = s_pAp;
    } else {
        pAp = sc->pAp;
    }
    if (!positive_finite(pAp)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { sc->pAp = pAp; cheb_publish_breakdown(f, sc->iteration, sc->rrNew, sc->rr0); }
        return;
    }
    const double alpha = sc->rr / pAp;
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc->pAp = pAp; sc->alpha = alpha; }   // alpha: for update_xp of this iteration
    const double malpha = -alpha;
    double acc = 0.0, accZ = 0.0;
    auto one = [&](long long i) {
        double u = malpha * Ap[i]; const double rv = r[i] + u; r[i] = rv;
        double q = rv * rv; acc += q;
        double dv = 0.0;
        if constexpr (DINV) dv = dinv[i];
        const double zv = cheb_first_term<DINV, RZ>(it, dv, rv, accZ);
        d[i] = zv; z[i] = zv;
    };
    if constexpr (V2) {
        d2* r2 = (d2*)r; const d2* a2 = (const d2*)Ap; const d2* d2p = (const d2*)dinv; d2* dd2 = (d2*)d; d2* z2 = (d2*)z;
        auto fin = [&](d2& rv, const d2& av, const d2& dv, d2& zv) {
            double u0 = malpha * av.x; double u1 = malpha * av.y; rv.x = rv.x + u0; rv.y = rv.y + u1;
            double q0 = rv.x * rv.x; double q1 = rv.y * rv.y; acc += q0; acc += q1;
            zv.x = cheb_first_term<DINV, RZ>(it, dv.x, rv.x, accZ); zv.y = cheb_first_term<DINV, RZ>(it, dv.y, rv.y, accZ);
        };
        chunk_pairs(n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            // Ap is not read again: streaming loads.  r, d and z come back in the steps that follow, z through the gathers: plain stores
            d2 av0 = ldv<NTV>(a2 + i), rv0 = r2[i], dv0 = {}, av1, rv1, dv1 = {}, zv0, zv1;
            if constexpr (DINV) dv0 = d2p[i];
            av1 = ldv<NTV>(a2 + j); rv1 = r2[j];
            if constexpr (DINV) dv1 = d2p[j];
            fin(rv0, av0, dv0, zv0); r2[i] = rv0; dd2[i] = zv0; z2[i] = zv0;
            if (two) { fin(rv1, av1, dv1, zv1); r2[j] = rv1; dd2[j] = zv1; z2[j] = zv1; }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
    const double t = block_sum(acc, s_red);                          // (s_red again: every wave has read the p.Ap sum, behind the barrier above)
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if constexpr (RZ) {
        __shared__ double s_red2[4];
        const double tz = block_sum(accZ, s_red2);
        if (threadIdx.x == 0) partialsZ[blockIdx.x] = tz;
    }
}
int launch_cheb_first(hipStream_t s, const FinalizeArgs& f, double* r, const double* Ap, const double* dinv, double* d, double* z, long long n, double it,
                      double* partials, double* partialsZ, bool withRz, const double* pApPartials, int nPAp)
{
    if (n < 0) n = 0;
    const bool v2 = al16(r) && al16(Ap) && al16(dinv) && al16(d) && al16(z);
    int grid = grid_for(n, v2 ? 4 : 2);
    DeviceState* dev = device_state();                                // update_r_kernel's grid: two workgroups per CU
    const int want = 2 * (dev ? dev->numCu : kNumCu);
    if (grid > want) grid = want;
    with_flags([&](auto V2, auto NTV, auto DINV, auto RZ) {
        hipLaunchKernelGGL((cheb_first_kernel<V2.value, NTV.value, DINV.value, RZ.value>), dim3(grid), dim3(kBlock), 0, s, f, r, Ap, dinv, d, z, n, it,
                           partials, partialsZ, pApPartials, nPAp);
    }, v2, vec_nt(n), dinv != nullptr, withRz);
    if (dot_reference_order()) {
        const int* done = &f.sc->done;
        launch_dot_serial(s, r, r, n, partials, done);
        if (withRz) launch_dot_serial(s, r, z, n, partialsZ, done);
        return 1;
    }
    return grid;
}

// ------------------------------------------------------------------ residual, stop test, r.z breakdown, beta (one workgroup)
// The stop rules judge the true residual of the iteration that just updated r; its x += alpha p is left to update_xp_kernel (pad = 1).
// Behind a decision to go on, an r.z that is not finite and > 0 ends the loop with MGCG_NONFINITE at the NEXT iteration's index: the
// iteration just judged is complete (update_xp_kernel still applies its x term), the next one cannot start.
__global__ __launch_bounds__(kBlock) void cheb_finalize_kernel(const double* __restrict__ partials, int n, const double* __restrict__ partialsZ, int nZ,
                                                               int reduceFirst, FinalizeArgs f)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    CgScalars* sc = f.sc;
    if (sc->done != 0) { if (threadIdx.x == 0) sc->pad = 0; return; }     // no iteration ran: nothing pending for update_xp
    double rrNew = 0.0, rzNew = 0.0;
    if (reduceFirst) {
        rrNew = reduce_partials_block(partials, n, s_red, 0);
        rzNew = reduce_partials_block(partialsZ, nZ, s_red2, 0);
    }
    if (threadIdx.x != 0) return;
    if (!reduceFirst) { rrNew = sc->rrNew; rzNew = sc->rzNew; }
    const int it = sc->iteration;
    const StopDecision d = decide_stop(f, rrNew, 0.0, sc->rr0, it);
    if (!d.stop && !positive_finite(rzNew)) {
        if (f.trace != nullptr && it < f.traceCap) f.trace[it] = d.shown;
        sc->rrNew = rrNew; sc->rzNew = rzNew; sc->nrmInf = 0; sc->pad = 1;
        cheb_publish_breakdown(f, it + 1, rrNew, sc->rr0);
        return;
    }
    publish_iteration<0>(f, d, it, rrNew, 0.0, 1, [&] { sc->rzNew = rzNew; sc->beta = rzNew / sc->rr; sc->rr = rzNew; });
}
void launch_cheb_finalize(hipStream_t s, const double* partials, int n, const double* partialsZ, int nZ, bool reduceFirst, const FinalizeArgs& f)
{
    hipLaunchKernelGGL(cheb_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, n, partialsZ, nZ, reduceFirst ? 1 : 0, f);
}

// ------------------------------------------------------------------ Gershgorin bound (MgcgGershgorinBound)
// The largest row sum of |a_ij| (times dinv_i) bounds the spectrum of A (of D^-1 A) from above.  A row is summed in stored order from +0.0;
// the maximum does not depend on the order it is taken in.  Offsets that run past the arrays: the row counts as what is stored.
__global__ __launch_bounds__(kBlock) void gershgorin_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets, long long nnz, long long n,
                                                            const double* __restrict__ dinv, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    double m = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        long long k = rowOffsets[i], end = rowOffsets[i + 1];
        if (k < 0) k = 0;
        if (end > nnz) end = nnz;
        double acc = 0.0;
        for (; k < end; ++k) { const double a = fabs(elements[k]); acc += a; }
        if (dinv != nullptr) acc = dinv[i] * acc;
        m = acc > m ? acc : m;
    });
    const double t = block_max(m, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
void launch_gershgorin(hipStream_t s, const double* elements, const int* rowOffsets, long long nnz, long long n, const double* dinv, double* partials, double* out)
{
    const int grid = grid_for(n, 1);
    hipLaunchKernelGGL(gershgorin_kernel, dim3(grid), dim3(kBlock), 0, s, elements, rowOffsets, nnz, n, dinv, partials);
    launch_reduce(s, partials, grid, out, 1);
}

void preload_kernels_cheb() { preload_code_object(reinterpret_cast<const void*>(&gershgorin_kernel)); }

} // namespace mgcg
