// BLAS-1 and fused CG vector updates for gfx950.
// Replaces cublasD{axpy,dot,scal,copy}_v2 (Mgcg/cuBlas/MgcgGpu/Mgcg.cu:22-54) and the OpenCL
// AddVectorVector / MultiplyVectorVector / ReductionSum / ReductionMaxAbsolute kernels
// (Mgcg/HandmadeCL/MgcgCL/Mgcg.cl:15-159).
//
// All kernels are grid-stride over a fixed grid (<= 8 workgroups of 256 threads per CU) with
// 16-byte loads when the operands allow it.  Element-wise arithmetic keeps the reference CPU
// twin's operation order (Mgcg/cuBlas/Mgcg/LongVector.cs:41-51: answer = left + a*right, product
// rounded first; the library is built with -ffp-contract=off), so x, r and p updates are
// bit-identical to it.  Reductions: per-lane partial -> __shfl_down over the 64-lane wavefront ->
// LDS across the 4 waves -> one partial per workgroup -> a single-workgroup second stage that adds
// the partials in a fixed order.  No atomics: results are run-to-run reproducible.
#include "vec_passes.hpp"

namespace mgcg {

// ------------------------------------------------------------------ axpy: y = y + alpha*x
template <bool V2>
__global__ __launch_bounds__(kBlock) void axpy_kernel(double* __restrict__ y, const double* __restrict__ x, long long n, double alpha)
{
    grid_stride<V2>(n,
        [&](long long i) { d2 xv = *(const d2*)(x + i); d2 yv = *(d2*)(y + i); d2 t; t.x = alpha * xv.x; t.y = alpha * xv.y; yv.x = yv.x + t.x; yv.y = yv.y + t.y; *(d2*)(y + i) = yv; },
        [&](long long i) { double t = alpha * x[i]; y[i] = y[i] + t; });
}
void launch_axpy(hipStream_t s, double* y, const double* x, long long n, double alpha)
{
    if (n <= 0) return;
    if (al16(y) && al16(x)) hipLaunchKernelGGL(axpy_kernel<true>, dim3(grid_for(n, 2)), dim3(kBlock), 0, s, y, x, n, alpha);
    else hipLaunchKernelGGL(axpy_kernel<false>, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, y, x, n, alpha);
}

// ------------------------------------------------------------------ scal: x = alpha*x
template <bool V2>
__global__ __launch_bounds__(kBlock) void scal_kernel(double* __restrict__ x, long long n, double alpha)
{
    grid_stride<V2>(n,
        [&](long long i) { d2 v = *(d2*)(x + i); v.x = alpha * v.x; v.y = alpha * v.y; *(d2*)(x + i) = v; },
        [&](long long i) { x[i] = alpha * x[i]; });
}
void launch_scal(hipStream_t s, double* x, double alpha, long long n)
{
    if (n <= 0) return;
    if (al16(x)) hipLaunchKernelGGL(scal_kernel<true>, dim3(grid_for(n, 2)), dim3(kBlock), 0, s, x, n, alpha);
    else hipLaunchKernelGGL(scal_kernel<false>, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, x, n, alpha);
}

// ------------------------------------------------------------------ xpay: y = x + beta*y   (Scal+Axpy of Mgcg.cu:197,265 fused)
template <bool V2>
__global__ __launch_bounds__(kBlock) void xpay_kernel(double* __restrict__ y, const double* __restrict__ x, long long n, double beta)
{
    grid_stride<V2>(n,
        [&](long long i) { d2 xv = *(const d2*)(x + i); d2 yv = *(d2*)(y + i); d2 t; t.x = beta * yv.x; t.y = beta * yv.y; yv.x = xv.x + t.x; yv.y = xv.y + t.y; *(d2*)(y + i) = yv; },
        [&](long long i) { double t = beta * y[i]; y[i] = x[i] + t; });
}
void launch_xpay(hipStream_t s, double* y, const double* x, long long n, double beta)
{
    if (n <= 0) return;
    if (al16(y) && al16(x)) hipLaunchKernelGGL(xpay_kernel<true>, dim3(grid_for(n, 2)), dim3(kBlock), 0, s, y, x, n, beta);
    else hipLaunchKernelGGL(xpay_kernel<false>, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, y, x, n, beta);
}

// ------------------------------------------------------------------ copy / fill
__global__ __launch_bounds__(kBlock) void fill_kernel(double* __restrict__ y, double v, long long n)
{
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { y[i] = v; });
}
void launch_copy(hipStream_t s, double* y, const double* x, long long n)
{
    if (n <= 0) return;
    (void)hipMemcpyAsync(y, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s);
}
void launch_fill(hipStream_t s, double* y, double v, long long n)
{
    if (n <= 0) return;
    if (v == 0.0) { (void)hipMemsetAsync(y, 0, (size_t)n * sizeof(double), s); return; }
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, y, v, n);
}

// ------------------------------------------------------------------ dot partials
// NT: streaming loads for vectors far larger than the caches (a pure read stream gains 4-10 % from them on this chip,
// profiles/r2/bw_probe.log; small vectors that the next kernel reads again keep the plain loads)
template <bool V2, bool NT = false>
__global__ __launch_bounds__(kBlock) void dot_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    double acc = 0.0;
    grid_stride<V2>(n,
        [&](long long i) {
            d2 xv, yv;
            if constexpr (NT) { xv = __builtin_nontemporal_load((const d2*)(x + i)); yv = __builtin_nontemporal_load((const d2*)(y + i)); }
            else { xv = *(const d2*)(x + i); yv = *(const d2*)(y + i); }
            double t0 = xv.x * yv.x; double t1 = xv.y * yv.y; acc += t0; acc += t1; },
        [&](long long i) { double t = x[i] * y[i]; acc += t; });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// ------------------------------------------------------------------ reference-order dot (validation mode: knob dot_order)
// The reference's CPU twin adds the rounded products strictly left to right (Mgcg/cuBlas/Mgcg/LongVector.cs:15-31) and the host adds
// the per-device sums in device order (ConjugateGradientParallelGpu.cs:463,499,525).  Everything element-wise in this library is
// already bit-identical to that twin; with dot_order = 1 every dot product of Dot / CsrMVDot / Solve / Solve0..2 / SolveParallel /
// SolveMg* takes this kernel instead of the tree sums, so whole residual traces and iterates become EQUAL to the oracle's, at any size
// and rank count.  One workgroup: waves 1-3 stage the rounded products of the next batch in LDS (coalesced) while lane 0 of wave 0
// adds the current batch in index order -- one dependent fp64 add per element, ~0.5 s per 1.3e8 entries.  A test instrument, never
// on a timed path.  (Padding a batch with +0.0 changes nothing: a running sum that started at +0.0 is never -0.0.)
constexpr int kSerialBatch = 2048;
// w (optional, the Jacobi-preconditioned loop's r.z without a stored z): the terms are x_i * (w_i * y_i), the inner product rounded first.
__global__ __launch_bounds__(kBlock) void dot_serial_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                            double* __restrict__ out, const int* done, const double* __restrict__ w)
{
    __shared__ double s_prod[2][kSerialBatch];
    if (done != nullptr && *done != 0) return;
    const int tid = threadIdx.x;
    const long long nBatches = (n + kSerialBatch - 1) / kSerialBatch;
    auto fill = [&](int buf, long long b) {
        const long long base = b * kSerialBatch;
        for (int k = tid - kWave; k < kSerialBatch; k += kBlock - kWave) {
            const long long i = base + k;
            double t = 0.0;
            if (i < n) {
                if (w != nullptr) { double z = w[i] * y[i]; t = x[i] * z; }
                else t = x[i] * y[i];
            }
            s_prod[buf][k] = t;
        }
    };
    if (tid >= kWave) fill(0, 0);
    __syncthreads();
    double acc = 0.0;
    for (long long b = 0; b < nBatches; ++b) {
        if (tid >= kWave) { if (b + 1 < nBatches) fill((int)((b + 1) & 1), b + 1); }
        else if (tid == 0) {
            const double* q = s_prod[b & 1];
#pragma unroll 16
            for (int k = 0; k < kSerialBatch; ++k) acc += q[k];
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = acc;
}
bool dot_reference_order() { return tuning().dotOrder.load(std::memory_order_relaxed) != 0; }
void launch_dot_serial(hipStream_t s, const double* x, const double* y, long long n, double* out, const int* done, const double* w)
{
    hipLaunchKernelGGL(dot_serial_kernel, dim3(1), dim3(kBlock), 0, s, x, y, n < 0 ? 0 : n, out, done, w);
}

int launch_dot_partials(hipStream_t s, const double* x, const double* y, long long n, double* partials)
{
    if (dot_reference_order()) { launch_dot_serial(s, x, y, n, partials, nullptr); return 1; }
    const bool v2 = al16(x) && al16(y);
    const int grid = grid_for(n, v2 ? 4 : 2);
    if (v2 && n >= (8LL << 20)) hipLaunchKernelGGL((dot_kernel<true, true>), dim3(grid), dim3(kBlock), 0, s, x, y, n, partials);
    else if (v2) hipLaunchKernelGGL((dot_kernel<true, false>), dim3(grid), dim3(kBlock), 0, s, x, y, n, partials);
    else hipLaunchKernelGGL((dot_kernel<false, false>), dim3(grid), dim3(kBlock), 0, s, x, y, n, partials);
    return grid;
}

__global__ __launch_bounds__(kBlock) void nrminf_kernel(const double* __restrict__ x, long long n, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    double m = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { double a = fabs(x[i]); m = a > m ? a : m; });
    const double t = block_max(m, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
int launch_nrminf_partials(hipStream_t s, const double* x, long long n, double* partials)
{
    const int grid = grid_for(n, 2);
    hipLaunchKernelGGL(nrminf_kernel, dim3(grid), dim3(kBlock), 0, s, x, n, partials);
    return grid;
}

// ------------------------------------------------------------------ second stage (one workgroup)
__global__ __launch_bounds__(kBlock) void reduce_kernel(const double* __restrict__ partials, int n, double* __restrict__ out, int mode, const int* done)
{
    __shared__ double s_red[4];
    if (done != nullptr && *done != 0) return;
    const double t = reduce_partials_block(partials, n, s_red, mode);
    if (threadIdx.x == 0) out[0] = t;
}
// partials[0] = sum / max of partials[0..n), in place (every read happens before the barrier inside the block reduction)
__global__ __launch_bounds__(kBlock) void reduce_inplace_kernel(double* partials, int n, int mode, const int* done)
{
    __shared__ double s_red[4];
    if (done != nullptr && *done != 0) return;
    const double t = reduce_partials_block(partials, n, s_red, mode);
    if (threadIdx.x == 0) partials[0] = t;
}
void launch_reduce(hipStream_t s, const double* partials, int n, double* out, int mode)
{
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kBlock), 0, s, partials, n, out, mode, (const int*)nullptr);
}
void launch_reduce_to(hipStream_t s, const double* partials, int n, double* dst, const int* done)
{
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kBlock), 0, s, partials, n, dst, 0, done);
}
// two sums in one launch (the preconditioned loop of several ranks: r.r and r.z in front of their one all-reduce), each in reduce_kernel's order
__global__ __launch_bounds__(kBlock) void reduce2_kernel(const double* __restrict__ pA, int nA, double* __restrict__ dstA,
                                                         const double* __restrict__ pB, int nB, double* __restrict__ dstB, const int* done)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    if (done != nullptr && *done != 0) return;
    const double ta = reduce_partials_block(pA, nA, s_red, 0);
    const double tb = reduce_partials_block(pB, nB, s_red2, 0);
    if (threadIdx.x == 0) { dstA[0] = ta; dstB[0] = tb; }
}
void launch_reduce2_to(hipStream_t s, const double* pA, int nA, double* dstA, const double* pB, int nB, double* dstB, const int* done)
{
    hipLaunchKernelGGL(reduce2_kernel, dim3(1), dim3(kBlock), 0, s, pA, nA, dstA, pB, nB, dstB, done);
}

// ------------------------------------------------------------------ fused CG pieces
// The Jacobi-preconditioned loop's share of r.z for one element, z = dinv * r rounded first (never contracted with the add that follows:
// product into a named double, then the add).  The r update and the x/p update both form z this way, so they see the same bits.
__device__ __forceinline__ double rz_term(double dinv, double r, double& acc) { double z = dinv * r; double t = r * z; acc += t; return z; }

// p = r ; partial r.r      DINV (the Jacobi-preconditioned loop's start): p = z = dinv * r ; partial r.r and r.z
template <bool V2, bool DINV>
__global__ __launch_bounds__(kBlock) void copy_dot_kernel(double* __restrict__ p, const double* __restrict__ r, const double* __restrict__ dinv, long long n,
                                                          double* __restrict__ partials, double* __restrict__ partialsZ, const int* done)
{
    __shared__ double s_red[4];
    if (done != nullptr && *done != 0) return;
    double acc = 0.0, accZ = 0.0;
    grid_stride<V2>(n,
        [&](long long i) {
            d2 rv = *(const d2*)(r + i), zv = rv;
            if constexpr (DINV) { d2 dv = *(const d2*)(dinv + i); zv.x = rz_term(dv.x, rv.x, accZ); zv.y = rz_term(dv.y, rv.y, accZ); }
            *(d2*)(p + i) = zv; double t0 = rv.x * rv.x; double t1 = rv.y * rv.y; acc += t0; acc += t1; },
        [&](long long i) { double rv = r[i], zv = rv; if constexpr (DINV) zv = rz_term(dinv[i], rv, accZ); p[i] = zv; double t = rv * rv; acc += t; });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if constexpr (DINV) {
        __shared__ double s_red2[4];
        const double tz = block_sum(accZ, s_red2);
        if (threadIdx.x == 0) partialsZ[blockIdx.x] = tz;
    }
}
int launch_copy_dot(hipStream_t s, double* p, const double* r, const double* dinv, long long n, double* partials, double* partialsZ, const int* done)
{
    const bool v2 = al16(p) && al16(r) && al16(dinv);
    const int grid = grid_for(n, v2 ? 4 : 2);
    with_flags([&](auto V2, auto DINV) {
        hipLaunchKernelGGL((copy_dot_kernel<V2.value, DINV.value>), dim3(grid), dim3(kBlock), 0, s, p, r, dinv, n, partials, partialsZ, done);
    }, v2, dinv != nullptr);
    if (dot_reference_order()) {                                      // the sums in the reference's order replace the partial sums
        launch_dot_serial(s, r, r, n, partials, done);
        if (dinv != nullptr) launch_dot_serial(s, r, r, n, partialsZ, done, dinv);
        return 1;
    }
    return grid;
}

// The element step of update_xr_kernel and update_r_kernel (one element, or the two halves of a 16-byte pair in turn), in two parts so
// that the callers can store r in between: r + (-alpha)*Ap with the product rounded first, then the new r's share of r.r and, with INF,
// of max|r|.
__device__ __forceinline__ double r_step(double malpha, double ap, double r) { double u = malpha * ap; return r + u; }
template <bool INF, typename... T>
__device__ __forceinline__ void r_sums(double& acc, double& mx, T... rv)
{
    const double q[] = { rv * rv... };
    for (double v : q) acc += v;
    if (INF) { const double a[] = { fabs(rv)... }; for (double v : a) mx = v > mx ? v : mx; }
}

// alpha = rr / pAp ; x = x + alpha*p ; r = r + (-alpha)*Ap ; partial r.r [, partial max|r|]
// (ConjugateGradientCpu.cs:71-74 in one pass over x, p, r, Ap)
template <bool V2, bool INF>
__global__ __launch_bounds__(kBlock) void update_xr_kernel(const CgScalars* __restrict__ sc, double* __restrict__ x, double* __restrict__ r,
                                                           const double* __restrict__ p, const double* __restrict__ Ap, long long n,
                                                           double* __restrict__ partials, double* __restrict__ partialsInf)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    if (sc->done != 0) return;
    const double alpha = sc->rr / sc->pAp;
    const double malpha = -alpha;
    double acc = 0.0, mx = 0.0;
    grid_stride<V2>(n,
        [&](long long i) {
            d2 pv = *(const d2*)(p + i); d2 xv = *(d2*)(x + i); d2 av = *(const d2*)(Ap + i); d2 rv = *(d2*)(r + i);
            double t0 = alpha * pv.x; double t1 = alpha * pv.y; xv.x = xv.x + t0; xv.y = xv.y + t1; *(d2*)(x + i) = xv;
            rv.x = r_step(malpha, av.x, rv.x); rv.y = r_step(malpha, av.y, rv.y); *(d2*)(r + i) = rv;
            r_sums<INF>(acc, mx, rv.x, rv.y);
        },
        [&](long long i) {
            double t = alpha * p[i]; x[i] = x[i] + t;
            double rv = r_step(malpha, Ap[i], r[i]); r[i] = rv;
            r_sums<INF>(acc, mx, rv);
        });
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if (INF) {
        const double m = block_max(mx, s_red2);
        if (threadIdx.x == 0) partialsInf[blockIdx.x] = m;
    }
}
int launch_update_xr(hipStream_t s, const CgScalars* sc, double* x, double* r, const double* p, const double* Ap,
                     long long n, double* partials, double* partialsInf)
{
    const bool v2 = al16(x) && al16(r) && al16(p) && al16(Ap);
    const int grid = grid_for(n, v2 ? 4 : 2);
    const bool inf = partialsInf != nullptr;
    with_flags([&](auto V2, auto INF) {
        hipLaunchKernelGGL((update_xr_kernel<V2.value, INF.value>), dim3(grid), dim3(kBlock), 0, s, sc, x, r, p, Ap, n, partials, partialsInf);
    }, v2, inf);
    if (dot_reference_order()) {
        launch_dot_serial(s, r, r, n, partials, nullptr);
        if (inf) hipLaunchKernelGGL(reduce_inplace_kernel, dim3(1), dim3(kBlock), 0, s, partialsInf, grid, 1, (const int*)nullptr);   // max of the partial maxima (order-free)
        return 1;
    }
    return grid;
}

// The device-resident loop splits the reference's update (ConjugateGradientCpu.cs:72-74,94) differently from the
// reference's phase functions: r first (its norm decides the stop test), then x and p together, so that p is read
// once for both x += alpha p and p = z + beta p  (64N bytes per iteration instead of 72N).
// alpha = rr / pAp ; r = r + (-alpha)*Ap ; partial r.r [, partial max|r|]
// DINV (the Jacobi-preconditioned loop, sc->rr holds r.z): one more load per element and the partial r.z of the rounded r with
// z = dinv * r (rz_term); dinv and partialsZ are null otherwise.  32 bytes per row (Ap, r, dinv in; r out) against 24.
template <bool V2, bool INF, bool NTV, bool DINV>
__global__ __launch_bounds__(kBlock) void update_r_kernel(CgScalars* __restrict__ sc, double* __restrict__ r, const double* __restrict__ Ap,
                                                          const double* __restrict__ dinv, long long n,
                                                          double* __restrict__ partials, double* __restrict__ partialsZ, double* __restrict__ partialsInf,
                                                          const double* __restrict__ pApPartials, int nPAp, int freeze)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    __shared__ double s_pAp;
    if (sc->done != 0) { if (freeze && blockIdx.x == 0 && threadIdx.x == 0) sc->fDone = 1; return; }   // tells the folded x/p update that no iteration ran
    double pAp;
    if (pApPartials != nullptr) {                                     // single-rank loop: no separate reduction launch
        const double t = reduce_partials_block(pApPartials, nPAp, s_red, 0);
        if (threadIdx.x == 0) s_pAp = t;
        __syncthreads();
        pAp = s_pAp;
        if (blockIdx.x == 0 && threadIdx.x == 0) sc->pAp = pAp;
    } else {
        pAp = sc->pAp;
    }
    const double alpha = sc->rr / pAp;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->alpha = alpha;                                            // for update_xp of this iteration
        if (freeze) { sc->fRr = sc->rr; sc->fRr0 = sc->rr0; sc->fAlpha = alpha; sc->fIteration = sc->iteration; sc->fDone = 0; }
    }
    const double malpha = -alpha;
    double acc = 0.0, accZ = 0.0, mx = 0.0;
    auto one = [&](long long i) {
        double rv = r_step(malpha, Ap[i], r[i]); r[i] = rv; r_sums<INF>(acc, mx, rv);
        if constexpr (DINV) (void)rz_term(dinv[i], rv, accZ);
    };
    if constexpr (V2) {
        d2* r2 = (d2*)r; const d2* a2 = (const d2*)Ap; const d2* d2p = (const d2*)dinv;
        auto fin = [&](d2& rv, const d2& av, const d2& dv) {
            rv.x = r_step(malpha, av.x, rv.x); rv.y = r_step(malpha, av.y, rv.y);
            r_sums<INF>(acc, mx, rv.x, rv.y);
            if constexpr (DINV) { (void)rz_term(dv.x, rv.x, accZ); (void)rz_term(dv.y, rv.y, accZ); }
        };
        chunk_pairs(n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            // streaming hints as in update_xp (measured there: 5.2 -> 6.3 TB/s): Ap is not read again, r not before 2 GB of other traffic
            // (DINV: r and dinv come back in the x/p update, after that pass's own 48 bytes per row)
            d2 av0 = ldv<NTV>(a2 + i), rv0 = ldv<NTV>(r2 + i), dv0 = {}, av1, rv1, dv1 = {};
            if constexpr (DINV) dv0 = ldv<NTV>(d2p + i);
            av1 = ldv<NTV>(a2 + j); rv1 = ldv<NTV>(r2 + j);
            if constexpr (DINV) dv1 = ldv<NTV>(d2p + j);
            fin(rv0, av0, dv0); stv<NTV>(rv0, r2 + i);
            if (two) { fin(rv1, av1, dv1); stv<NTV>(rv1, r2 + j); }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if constexpr (DINV) {
        __shared__ double s_red3[4];
        const double tz = block_sum(accZ, s_red3);
        if (threadIdx.x == 0) partialsZ[blockIdx.x] = tz;
    }
    if (INF) {
        const double m = block_max(mx, s_red2);
        if (threadIdx.x == 0) partialsInf[blockIdx.x] = m;
    }
}
int launch_update_r(hipStream_t s, CgScalars* sc, double* r, const double* Ap, const double* dinv, long long n, double* partials, double* partialsZ,
                    double* partialsInf, const double* pApPartials, int nPAp, bool freeze)
{
    const bool v2 = al16(r) && al16(Ap) && al16(dinv);
    int grid = grid_for(n, v2 ? 4 : 2);
    // two workgroups per CU measured best for this 2-reads-1-write pass (0.565 ms against 0.59-0.61 for 768 / 1024 / 2048 and 0.72 for 256
    // workgroups at 512^3; the 3-reads-2-writes x/p pass keeps 2048)
    DeviceState* d = device_state();
    const int want = 2 * (d ? d->numCu : kNumCu);
    if (grid > want) grid = want;
    const bool inf = partialsInf != nullptr;
    with_flags([&](auto V2, auto INF, auto NTV, auto DINV) {
        hipLaunchKernelGGL((update_r_kernel<V2.value, INF.value, NTV.value, DINV.value>), dim3(grid), dim3(kBlock), 0, s, sc, r, Ap, dinv, n, partials, partialsZ, partialsInf,
                           pApPartials, nPAp, freeze ? 1 : 0);
    }, v2, inf, vec_nt(n), dinv != nullptr);
    if (dot_reference_order()) {
        launch_dot_serial(s, r, r, n, partials, &sc->done);
        if (dinv != nullptr) launch_dot_serial(s, r, r, n, partialsZ, &sc->done, dinv);
        if (inf) hipLaunchKernelGGL(reduce_inplace_kernel, dim3(1), dim3(kBlock), 0, s, partialsInf, grid, 1, (const int*)&sc->done);
        return 1;
    }
    return grid;
}

// The element pass of update_xp_kernel and update_xp_final_kernel: x = x + alpha*p and, unless this iteration stopped the loop (stop: x
// only), p = z + beta*p.  Every product is rounded, then added; p is read once for both.  DINV (the Jacobi-preconditioned loop): the
// caller passes r for z and z_i = dinv_i * r_i is formed here, the bits update_r summed (48 bytes per row against 40); dinv is null otherwise.
template <bool V2, bool NTV, bool DINV>
__device__ __forceinline__ void xp_pass(double alpha, double beta, bool stop, double* __restrict__ x, double* __restrict__ p, const double* __restrict__ z,
                                        const double* __restrict__ dinv, long long n)
{
    if (stop) {
        grid_stride<V2>(n,
            [&](long long i) { d2 pv = *(const d2*)(p + i); d2 xv = *(d2*)(x + i); double t0 = alpha * pv.x; double t1 = alpha * pv.y; xv.x = xv.x + t0; xv.y = xv.y + t1; *(d2*)(x + i) = xv; },
            [&](long long i) { double t = alpha * p[i]; x[i] = x[i] + t; });
        return;
    }
    auto one = [&](long long i) {
        const double pv = p[i]; double t = alpha * pv; x[i] = x[i] + t;
        double zv = z[i];
        if constexpr (DINV) zv = dinv[i] * zv;
        double u = beta * pv; p[i] = zv + u;
    };
    if constexpr (V2) {
        // streaming hints on both sides: none of x, p, z is touched again before ~2 GB of other traffic
        d2* x2 = (d2*)x; d2* p2 = (d2*)p; const d2* z2 = (const d2*)z; const d2* d2p = (const d2*)dinv;
        auto fin = [&](d2& xv, d2& pv, const d2& zv, const d2& dv) {
            double t0 = alpha * pv.x; double t1 = alpha * pv.y; xv.x = xv.x + t0; xv.y = xv.y + t1;
            double z0 = zv.x, z1 = zv.y;
            if constexpr (DINV) { z0 = dv.x * zv.x; z1 = dv.y * zv.y; }
            double u0 = beta * pv.x; double u1 = beta * pv.y; pv.x = z0 + u0; pv.y = z1 + u1;
        };
        chunk_pairs(n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            d2 pv0 = ldv<NTV>(p2 + i), xv0 = ldv<NTV>(x2 + i), zv0 = ldv<NTV>(z2 + i), dv0 = {}, dv1 = {};
            if constexpr (DINV) dv0 = ldv<NTV>(d2p + i);
            d2 pv1 = ldv<NTV>(p2 + j), xv1 = ldv<NTV>(x2 + j), zv1 = ldv<NTV>(z2 + j);
            if constexpr (DINV) dv1 = ldv<NTV>(d2p + j);
            fin(xv0, pv0, zv0, dv0);
            stv<NTV>(xv0, x2 + i); stv<NTV>(pv0, p2 + i);
            if (two) { fin(xv1, pv1, zv1, dv1); stv<NTV>(xv1, x2 + j); stv<NTV>(pv1, p2 + j); }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

// x = x + alpha*p (whenever the iteration ran: sc->pad is the finalisation kernel's "x pending" mark) and, unless the
// stop test fired, p = z + beta*p.
template <bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void update_xp_kernel(const CgScalars* __restrict__ sc, double* __restrict__ x, double* __restrict__ p,
                                                           const double* __restrict__ z, long long n)
{
    if (sc->pad == 0) return;                   // this iteration did not run (the loop had already stopped)
    const double alpha = sc->alpha, beta = sc->beta;
    xp_pass<V2, NTV, false>(alpha, beta, sc->done != 0, x, p, z, nullptr, n);   // (done: this is the iteration that stopped the loop)
}
void launch_update_xp(hipStream_t s, const CgScalars* sc, double* x, double* p, const double* z, long long n)
{
    if (n <= 0) return;
    const bool v2 = al16(x) && al16(p) && al16(z);
    with_v2_nt(v2, vec_nt(n), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((update_xp_kernel<V2.value, NTV.value>), dim3(grid_for(n, V2.value ? 2 : 1)), dim3(kBlock), 0, s, sc, x, p, z, n);
    });
}


// The finalisation that the x/p updates below fold in.  Every workgroup reduces the r.r (and max|r|) partial sums of update_r in the order
// finalize_kernel uses and takes the same decision from the values update_r froze (fRr, fRr0, fAlpha, fIteration); workgroup 0 alone
// rewrites the live scalars, the host mirror and the trace, which nothing in these kernels reads.  beta and the decision reach the other
// lanes through LDS.  ALLREDUCED: the kernel also serves several ranks, where nPartials == 0 says that r.r has been reduced and
// all-reduced into sc->rrNew before the launch (workgroup 0 writes the same bits back).  RING_NT > 0: the deferred x update's two stores.
// PRECOND (the Jacobi-preconditioned loop): the r.z partial sums (partialsZ, or the all-reduced sc->rzNew) are reduced as well; the stop
// test keeps the true r.r against the true r0.r0 in fRr0, while beta = rzNew / rz and the hand-over take r.z (rz lives in sc->rr / fRr).
struct FrozenStep { double alpha, beta; bool stop; };
template <bool ALLREDUCED, int RING_NT, bool PRECOND = false>
__device__ __forceinline__ FrozenStep finalize_frozen(const FinalizeArgs& f, const double* partials, const double* partialsInf, int nPartials,
                                                      const double* partialsZ = nullptr)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    __shared__ double s_beta;
    __shared__ int s_stop;
    CgScalars* sc = f.sc;
    const double rrNew = (!ALLREDUCED || nPartials > 0) ? reduce_partials_block(partials, nPartials, s_red, 0) : sc->rrNew;
    double inf = 0.0;
    if (partialsInf != nullptr && (!ALLREDUCED || nPartials > 0)) inf = reduce_partials_block(partialsInf, nPartials, s_red2, 1);
    double rzNew = 0.0;
    if constexpr (PRECOND) {
        __shared__ double s_red3[4];
        rzNew = (!ALLREDUCED || nPartials > 0) ? reduce_partials_block(partialsZ, nPartials, s_red3, 0) : sc->rzNew;
    }
    const double alpha = sc->fAlpha;
    if (threadIdx.x == 0) {
        const int it = sc->fIteration;
        const StopDecision d = decide_stop(f, rrNew, inf, sc->fRr0, it);
        const double handOver = PRECOND ? rzNew : rrNew;
        const double beta = handOver / sc->fRr;
        s_stop = d.stop ? 1 : 0; s_beta = beta;
        if (blockIdx.x == 0)
            publish_iteration<RING_NT>(f, d, it, rrNew, inf, 0, [&] {
                if constexpr (RING_NT > 0) sc->alphaRing[RING_NT - 1] = alpha;   // (read by this group's later iterations only: no workgroup here reads it)
                if constexpr (PRECOND) sc->rzNew = rzNew;
                sc->beta = beta; sc->rr = handOver;
            });
    }
    __syncthreads();
    return { alpha, s_beta, s_stop != 0 };
}

// The x/p update with the iteration's finalisation folded in (one rank, or several behind their all-reduce of r.r).  Needs update_r
// launched with freeze = true.  The arithmetic of x and p is update_xp_kernel's.  No preconditioner: z = r.  DINV (the Jacobi-preconditioned
// loop): the finalisation takes beta from r.z (partialsZ, or with nPartials == 0 the all-reduced pair {rrNew, rzNew}) and z = dinv * r.
template <bool V2, bool NTV, bool DINV>
__global__ __launch_bounds__(kBlock) void update_xp_final_kernel(FinalizeArgs f, const double* __restrict__ partials, const double* __restrict__ partialsZ,
                                                                 const double* __restrict__ partialsInf, int nPartials, double* __restrict__ x,
                                                                 double* __restrict__ p, const double* __restrict__ r, const double* __restrict__ dinv, long long n)
{
    CgScalars* sc = f.sc;
    if (sc->fDone != 0) return;                                       // the loop had stopped before this iteration: nothing ran, nothing is pending
    const FrozenStep k = finalize_frozen<true, 0, DINV>(f, partials, partialsInf, nPartials, partialsZ);
    xp_pass<V2, NTV, DINV>(k.alpha, k.beta, k.stop, x, p, r, dinv, n);
}
void launch_update_xp_final(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsZ, const double* partialsInf, int nPartials,
                            double* x, double* p, const double* r, const double* dinv, long long n)
{
    if (n <= 0) return;
    const bool v2 = al16(x) && al16(p) && al16(r) && al16(dinv);
    with_v2_nt(v2, vec_nt(n), [&](auto V2, auto NTV) {
        with_flags([&](auto DINV) {
            hipLaunchKernelGGL((update_xp_final_kernel<V2.value, NTV.value, DINV.value>), dim3(grid_for(n, V2.value ? 2 : 1)), dim3(kBlock), 0, s, f, partials, partialsZ,
                               partialsInf, nPartials, x, p, r, dinv, n);
        }, dinv != nullptr);
    });
}

// The same with the deferred x update (RingArgs, common.hpp): the finalisation and stop decision of update_xp_final_kernel, then
// p_{k+1} = z + beta p_k from slot[pos] into the next slot.  The group's last iteration (flush) and the iteration that stops the loop also
// apply the NT = pos + 1 pending terms to x, oldest first; the other iterations do not touch x (24N bytes instead of 40N).  The slots may
// alias (the flush writes slot 0 in place, pos = 0 reads and writes slot 0): every element is read before it is written, by the same lane.
// FLUSH (the host knows which iterations close a group) compiles the unrolled form of the x terms, all loads in flight together (130 VGPRs
// at NT = 8); the other iterations keep the register count of the p-only pass and apply the terms one slot after another when the stop
// test fires in them (once per solve).
template <bool V2, bool NTV, int NT, bool FLUSH>
__global__ __launch_bounds__(kBlock) void update_xp_ring_kernel(FinalizeArgs f, const double* __restrict__ partials, const double* __restrict__ partialsInf,
                                                                int nPartials, double* __restrict__ x, RingArgs g, const double* __restrict__ z, long long n)
{
    CgScalars* sc = f.sc;
    if (sc->fDone != 0) return;                                       // the loop had stopped before this iteration: nothing ran, nothing is pending
    const FrozenStep k = finalize_frozen<false, NT>(f, partials, partialsInf, nPartials);
    const double alpha = k.alpha, beta = k.beta;
    const bool stop = k.stop;
    const double* pk = g.slot[NT - 1];
    double* pn = g.slot[(FLUSH || NT == kXDeferMax) ? 0 : NT];
    if (!FLUSH && stop) {                                             // stopped inside a group: x only, one term after another
        for (int t = 0; t < NT; ++t) {
            const double at = t < NT - 1 ? sc->alphaRing[t] : alpha;
            const double* pt = g.slot[t];
            grid_stride<false>(n, [&](long long) {}, [&](long long i) { double u = at * pt[i]; x[i] = x[i] + u; });
        }
        return;
    }
    if (FLUSH) {
        double al[NT];
#pragma unroll
        for (int t = 0; t < NT - 1; ++t) al[t] = sc->alphaRing[t];
        al[NT - 1] = alpha;
        auto one = [&](long long i) {
            double xv = x[i];
#pragma unroll
            for (int t = 0; t < NT; ++t) { double u = al[t] * g.slot[t][i]; xv = xv + u; }
            x[i] = xv;
            if (!stop) { double u = beta * pk[i]; pn[i] = z[i] + u; }
        };
        if constexpr (V2) {
            d2* x2 = (d2*)x; d2* pn2 = (d2*)pn; const d2* z2 = (const d2*)z;
            auto fin = [&](d2& xv, const d2* pv) {
#pragma unroll
                for (int t = 0; t < NT; ++t) { double u0 = al[t] * pv[t].x; double u1 = al[t] * pv[t].y; xv.x = xv.x + u0; xv.y = xv.y + u1; }
            };
            chunk_pairs(n >> 1, [&](long long i, bool two) {
                const long long j = two ? i + kBlock : i;
                d2 pv0[NT], pv1[NT];
                d2 xv0 = ldv<NTV>(x2 + i), xv1 = ldv<NTV>(x2 + j);
#pragma unroll
                for (int t = 0; t < NT; ++t) { pv0[t] = ldv<NTV>((const d2*)g.slot[t] + i); pv1[t] = ldv<NTV>((const d2*)g.slot[t] + j); }
                d2 zv0 = {}, zv1 = {};
                if (!stop) { zv0 = ldv<NTV>(z2 + i); zv1 = ldv<NTV>(z2 + j); }
                fin(xv0, pv0);
                stv<NTV>(xv0, x2 + i);
                if (!stop) { double u0 = beta * pv0[NT - 1].x; double u1 = beta * pv0[NT - 1].y; zv0.x = zv0.x + u0; zv0.y = zv0.y + u1; stv<NTV>(zv0, pn2 + i); }
                if (two) {
                    fin(xv1, pv1);
                    stv<NTV>(xv1, x2 + j);
                    if (!stop) { double u0 = beta * pv1[NT - 1].x; double u1 = beta * pv1[NT - 1].y; zv1.x = zv1.x + u0; zv1.y = zv1.y + u1; stv<NTV>(zv1, pn2 + j); }
                }
            });
            if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
        } else {
            grid_stride<false>(n, [&](long long) {}, one);
        }
        return;
    }
    auto one = [&](long long i) { double u = beta * pk[i]; pn[i] = z[i] + u; };
    if constexpr (V2) {
        const d2* pk2 = (const d2*)pk; d2* pn2 = (d2*)pn; const d2* z2 = (const d2*)z;
        chunk_pairs(n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            d2 pv0 = ldv<NTV>(pk2 + i), zv0 = ldv<NTV>(z2 + i), pv1 = ldv<NTV>(pk2 + j), zv1 = ldv<NTV>(z2 + j);
            double u0 = beta * pv0.x; double u1 = beta * pv0.y; zv0.x = zv0.x + u0; zv0.y = zv0.y + u1;
            stv<NTV>(zv0, pn2 + i);
            if (two) { u0 = beta * pv1.x; u1 = beta * pv1.y; zv1.x = zv1.x + u0; zv1.y = zv1.y + u1; stv<NTV>(zv1, pn2 + j); }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}
template <int NT, bool FLUSH>
static void launch_xp_ring_nt2(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsInf, int nPartials,
                               double* x, const RingArgs& g, const double* z, long long n, bool v2, bool nt)
{
    // the p-only pass (2 reads, 1 write: update_r's shape) takes update_r's two workgroups per CU -- 570-578 us against 597-598 for 2048
    // workgroups at 512^3 (profiles/r6/ring_grid_ab.txt); the flush (B + 2 reads, 2 writes) keeps the x/p pass's 2048
    int g2 = grid_for(n, 2);
    if (!FLUSH) { DeviceState* d = device_state(); const int want = 2 * (d ? d->numCu : kNumCu); if (g2 > want) g2 = want; }
    with_v2_nt(v2, nt, [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((update_xp_ring_kernel<V2.value, NTV.value, NT, FLUSH>), dim3(V2.value ? g2 : grid_for(n, 1)), dim3(kBlock), 0, s, f, partials, partialsInf, nPartials, x, g, z, n);
    });
}
template <int NT>
static void launch_xp_ring_nt(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsInf, int nPartials,
                              double* x, const RingArgs& g, const double* z, long long n, bool v2, bool nt)
{
    if (g.flush || NT == kXDeferMax) launch_xp_ring_nt2<NT, true>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt);
    else launch_xp_ring_nt2<NT, false>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt);
}
void launch_update_xp_ring(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsInf, int nPartials,
                           double* x, const RingArgs& g, const double* z, long long n)
{
    if (n <= 0) return;
    bool v2 = al16(x) && al16(z);
    for (int t = 0; t <= g.pos + 1 && t < kXDeferMax; ++t) v2 = v2 && al16(g.slot[t]);
    const bool nt = vec_nt(n);
    static_assert(kXDeferMax == 8, "one instantiation per position in the group");
    switch (g.pos) {
    case 0: launch_xp_ring_nt<1>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 1: launch_xp_ring_nt<2>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 2: launch_xp_ring_nt<3>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 3: launch_xp_ring_nt<4>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 4: launch_xp_ring_nt<5>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 5: launch_xp_ring_nt<6>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    case 6: launch_xp_ring_nt<7>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    default: launch_xp_ring_nt<8>(s, f, partials, partialsInf, nPartials, x, g, z, n, v2, nt); break;
    }
}

// p back into slot 0 after a call that stopped inside a group (sc->pSlot: the slot that holds it; 0: nothing to do)
__global__ __launch_bounds__(kBlock) void ring_copy_back_kernel(const CgScalars* __restrict__ sc, RingArgs g, long long n)
{
    const int from = sc->pSlot;
    if (from <= 0 || from >= kXDeferMax) return;
    const double* src = g.slot[from];
    double* dst = g.slot[0];
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { dst[i] = src[i]; });
}
void launch_ring_copy_back(hipStream_t s, const CgScalars* sc, const RingArgs& g, long long n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(ring_copy_back_kernel, dim3(grid_for(n, 4)), dim3(kBlock), 0, s, sc, g, n);
}

// ------------------------------------------------------------------ scalar bookkeeping (one workgroup)
// The scalars in front of iteration 0.  rr: what alpha and beta divide (r.r, or r.z of a preconditioned loop); rr0: what the relative
// stop rule divides by (the true r0.r0).
__device__ __forceinline__ void reset_scalars(CgScalars* sc, HostMirror* mirror, double rr, double rr0)
{
    sc->rr = rr; sc->rr0 = rr0; sc->pAp = 0; sc->rrNew = 0; sc->rzNew = 0; sc->residual = 0; sc->nrmInf = 0;
    sc->beta = 0; sc->alpha = 0; sc->iteration = 0; sc->done = 0; sc->status = 0; sc->pad = 0;
    sc->fRr = rr; sc->fRr0 = rr0; sc->fAlpha = 0; sc->fIteration = 0; sc->fDone = 0; sc->pSlot = 0;
    mirror->residual = 0; mirror->iteration = 0; mirror->status = 0; mirror->done = 0;
}
// partialsZ (the Jacobi-preconditioned loop, else null): rz = r0.z0 goes where alpha and beta look for it, the true r0.r0 where the relative
// rule does.  !reduceFirst (several ranks): the sums are all-reduced already, r.r in sc->rr, or with partialsZ the pair in {sc->rrNew, sc->rzNew}.
__global__ __launch_bounds__(kBlock) void init_scalars_kernel(const double* __restrict__ partials, const double* __restrict__ partialsZ, int n, int reduceFirst,
                                                              CgScalars* sc, HostMirror* mirror)
{
    __shared__ double s_red[4];
    const bool precond = partialsZ != nullptr;
    double rr = 0.0, rz = 0.0;
    if (reduceFirst) {
        rr = reduce_partials_block(partials, n, s_red, 0);
        if (precond) { __syncthreads(); rz = reduce_partials_block(partialsZ, n, s_red, 0); }   // (s_red again: every wave has read the first sum)
    }
    if (threadIdx.x == 0) {
        if (!reduceFirst) { rr = precond ? sc->rrNew : sc->rr; rz = sc->rzNew; }
        reset_scalars(sc, mirror, precond ? rz : rr, rr);
    }
}
void launch_init_scalars(hipStream_t s, const double* partials, const double* partialsZ, int n, bool reduceFirst, CgScalars* sc, HostMirror* mirror)
{
    hipLaunchKernelGGL(init_scalars_kernel, dim3(1), dim3(kBlock), 0, s, partials, partialsZ, n, reduceFirst ? 1 : 0, sc, mirror);
}

// Residual, stop test, beta and the rr hand-over.
__global__ __launch_bounds__(kBlock) void finalize_kernel(const double* __restrict__ partials, const double* __restrict__ partialsInf, int n,
                                                          int reduceFirst, FinalizeArgs f)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    CgScalars* sc = f.sc;
    if (sc->done != 0) { if (threadIdx.x == 0) sc->pad = 0; return; }     // no iteration ran: nothing pending for update_xp
    double rrNew = 0.0, inf = 0.0;
    if (reduceFirst) {
        rrNew = reduce_partials_block(partials, n, s_red, 0);
        if (partialsInf != nullptr) inf = reduce_partials_block(partialsInf, n, s_red2, 1);
    }
    if (threadIdx.x != 0) return;
    if (!reduceFirst) { rrNew = sc->rrNew; inf = sc->nrmInf; }
    const int it = sc->iteration;
    const StopDecision d = decide_stop(f, rrNew, inf, sc->rr0, it);
    publish_iteration<0>(f, d, it, rrNew, inf, 1, [&] {                                                         // pad = 1: x += alpha p is left to update_xp
        if (!f.preconditioned) { sc->beta = rrNew / sc->rr; sc->rr = rrNew; }
        else if (f.preconditioned == 2) { const double rz = sc->rzNew; sc->beta = rz / sc->rr; sc->rr = rz; }   // (all-reduced r.z already in place)
    });
}
void launch_finalize(hipStream_t s, const double* partials, const double* partialsInf, int n, bool reduceFirst, const FinalizeArgs& f)
{
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, partialsInf, n, reduceFirst ? 1 : 0, f);
}

// Preconditioned loop: rzNew = r.z ; beta = rzNew / rz ; rz = rzNew   (rz lives in sc->rr)
__global__ __launch_bounds__(kBlock) void finalize_precond_kernel(const double* __restrict__ partials, int n, int reduceFirst, CgScalars* sc)
{
    __shared__ double s_red[4];
    if (sc->done != 0) return;
    double rz = 0.0;
    if (reduceFirst) rz = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    if (!reduceFirst) rz = sc->rzNew;
    sc->rzNew = rz;
    sc->beta = rz / sc->rr;
    sc->rr = rz;
}
void launch_finalize_precond(hipStream_t s, const double* partials, int n, bool reduceFirst, CgScalars* sc)
{
    hipLaunchKernelGGL(finalize_precond_kernel, dim3(1), dim3(kBlock), 0, s, partials, n, reduceFirst ? 1 : 0, sc);
}

// ------------------------------------------------------------------ Jacobi-preconditioned loop (SolveJacobi / SolveJacobiParallel)
// z = D^-1 r is element-wise, so the preconditioned iteration keeps the plain loop's two launches after the product and stores no z:
// the DINV forms of copy_dot_kernel, update_r_kernel and update_xp_final_kernel above form z_i = dinv_i * r_i themselves (rz_term).  The r
// update moves 32 bytes per row, the x/p update 48: 80 against the plain loop's 64.  What is left here is the set-up.

// dinv_i = 1 / a_ii, a_ii = the first stored entry of local row i in column rowBase + i (rows need not be sorted).  A row without that
// entry, or with one that is not finite and > 0 (or so small that its reciprocal is not finite), raises bad[0] and lowers bad[1] to its index (pre-set to {0, INT_MAX} by the caller).
__global__ __launch_bounds__(kBlock) void jacobi_setup_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                              long long nnz, long long n, long long rowBase, double* __restrict__ dinv, int* bad)
{
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        long long k = rowOffsets[i], end = rowOffsets[i + 1];
        if (k < 0) k = 0;
        if (end > nnz) end = nnz;                                      // (offsets that run past the arrays: the row counts as what is stored)
        double d = 0.0;
        for (; k < end; ++k) if (columnIndeces[k] == rowBase + i) { d = elements[k]; break; }
        const double inv = 1.0 / d;
        if (d > 0.0 && isfinite(d) && isfinite(inv)) dinv[i] = inv;    // (no entry: d = 0; a subnormal diagonal, whose reciprocal overflows, fails as well)
        else { bad[0] = 1; atomicMin(&bad[1], (int)i); }
    });
}
void launch_jacobi_setup(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long nnz, long long n, long long rowBase,
                         double* dinv, int* bad)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(jacobi_setup_kernel, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, elements, rowOffsets, columnIndeces, nnz, n, rowBase, dinv, bad);
}

void preload_kernels_blas1() { preload_code_object(reinterpret_cast<const void*>(&fill_kernel)); }

} // namespace mgcg
