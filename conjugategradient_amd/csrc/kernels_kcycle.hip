// The K-cycle of the aggregation multigrid (gfx950; MgSetCycle(mg, 1, inner)): the vector passes of the K step, Notay's two Krylov steps
// preconditioned by the cycle in place of one coarse cycle.  The contract -- the formulas, their roundings and the breakdown rules -- is
// written out in include/MgcgGpu.h; tests/test_kcycle_host.py states it in numpy and under dot_order = 1 the passes here must EQUAL it.
// solver.hip's mg_kstep enqueues them between the two cycles and the two products v = A_C c (the level's own launch_spmv_auto).
//
// Every vector has the rows n of the coarse level C.  Per K step, vectors read + written:
//     sums 1     kcycle_sums1_kernel      the partial sums of rho1 = u1.v1 and beta1 = u1.b         reads c1 (inner 0 only), v1, b          3 / 2
//     residual   kcycle_residual_kernel   a1 = beta1 / rho1 ; rr = b - a1 v1                        reads b, v1, writes rr                  3
//     sums 2     kcycle_sums2_kernel      the partial sums of gamma = u2.v1, beta = u2.v2, a2 = u2.rr   reads c2 (inner 0 only), v2, v1, rr 4 / 3
//     combine    kcycle_combine_kernel    rho2, k1, k2 ; e = k1 c1 + k2 c2                          reads c1, c2, writes e                  3
// 13 (inner = 0) or 11 (inner = 1) vectors of 8 n bytes, beside the two cycles and the two products.  u(c, v) = c (inner = 0: the conjugate form)
// or v (inner = 1: the minimal-residual form) is a template flag of the two sums passes.
// No scalar is stored: every workgroup of the residual and the combine pass adds the per-workgroup partial sums in front of it in index
// order (reduce_partials_block, as the combine pass of kernels_bicgstabl.hip does) and keeps its own copy of a1, rho2, k1 and k2 in
// registers -- five fixed-order sums of at most kMaxGrid doubles against a launch and its drain on the critical path of a small level.  All
// workgroups take the same breakdown decision from the same sums.  Under dot_order = 1 the sums are launch_dot_serial's, one partial each.
// No atomics; -ffp-contract=off: every product is rounded before the sum or difference that takes it.
#include "vec_passes.hpp"

namespace mgcg {

// region q of a level's partial sums: 0 rho1, 1 beta1, 2 gamma, 3 beta, 4 a2
static double* kcycle_region(double* partials, int q) { return partials + (size_t)q * kMaxGrid; }

template <bool INNER>
__global__ __launch_bounds__(kBlock) void kcycle_sums1_kernel(const double* __restrict__ c1, const double* __restrict__ v1, const double* __restrict__ b,
                                                              long long n, double* __restrict__ partials, const int* done)
{
    __shared__ double s_red[2][4];
    if (done != nullptr && *done != 0) return;
    double accRho = 0.0, accBeta = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double v = v1[i];
        const double u = INNER ? v : c1[i];
        const double p = u * v; accRho += p;
        const double q = u * b[i]; accBeta += q;
    }
    const double rho = block_sum(accRho, s_red[0]);
    const double beta = block_sum(accBeta, s_red[1]);
    if (threadIdx.x == 0) { partials[blockIdx.x] = rho; partials[(size_t)kMaxGrid + blockIdx.x] = beta; }
}

template <bool INNER>
__global__ __launch_bounds__(kBlock) void kcycle_sums2_kernel(const double* __restrict__ c2, const double* __restrict__ v2, const double* __restrict__ v1,
                                                              const double* __restrict__ rr, long long n, double* __restrict__ partials, const int* done)
{
    __shared__ double s_red[3][4];
    if (done != nullptr && *done != 0) return;
    double accGamma = 0.0, accBeta = 0.0, accA2 = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double v = v2[i];
        const double u = INNER ? v : c2[i];
        const double p = u * v1[i]; accGamma += p;
        const double q = u * v; accBeta += q;
        const double t = u * rr[i]; accA2 += t;
    }
    const double gamma = block_sum(accGamma, s_red[0]);
    const double beta = block_sum(accBeta, s_red[1]);
    const double a2 = block_sum(accA2, s_red[2]);
    if (threadIdx.x == 0) {
        partials[(size_t)2 * kMaxGrid + blockIdx.x] = gamma; partials[(size_t)3 * kMaxGrid + blockIdx.x] = beta; partials[(size_t)4 * kMaxGrid + blockIdx.x] = a2;
    }
}

// rr = b - a1 v1, or b itself when rho1 is not finite or not > 0 (b = 0 among the causes: rr = b, never NaN)
__global__ __launch_bounds__(kBlock) void kcycle_residual_kernel(const double* __restrict__ b, const double* __restrict__ v1, double* __restrict__ rr, long long n,
                                                                 const double* __restrict__ partials, int nPartials, const int* done)
{
    __shared__ double s_red[2][4];
    if (done != nullptr && *done != 0) return;
    const double rho1 = reduce_partials_block(partials, nPartials, s_red[0], 0);
    const double beta1 = reduce_partials_block(partials + kMaxGrid, nPartials, s_red[1], 0);
    const bool live = positive_finite(rho1);
    const double a1 = beta1 / rho1;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double bi = b[i];
        const double av = a1 * v1[i];
        rr[i] = live ? bi - av : bi;
    }
}

// e = k1 c1 + k2 c2; c1 when rho1 broke down (the V-cycle's answer), a1 c1 when rho2 did.  e may be c2's own buffer: a lane reads its
// element of c2 before it writes that element of e.
__global__ __launch_bounds__(kBlock) void kcycle_combine_kernel(const double* __restrict__ c1, const double* c2, double* e, long long n,
                                                                const double* __restrict__ partials, int nPartials, const int* done)
{
    __shared__ double s_red[5][4];
    if (done != nullptr && *done != 0) return;
    double sum[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) sum[q] = reduce_partials_block(partials + (size_t)q * kMaxGrid, nPartials, s_red[q], 0);
    const double rho1 = sum[0], beta1 = sum[1], gamma = sum[2], beta = sum[3], a2 = sum[4];
    const bool live1 = positive_finite(rho1);
    const double a1 = beta1 / rho1;
    const double t = gamma * gamma;
    const double tq = t / rho1;
    const double rho2 = beta - tq;
    const bool live2 = live1 && positive_finite(rho2);
    const double ga = gamma * a2;
    const double rp = rho1 * rho2;
    const double gq = ga / rp;
    const double k1 = a1 - gq;
    const double k2 = a2 / rho2;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double x1 = c1[i], x2 = c2[i];
        const double p1 = k1 * x1;
        const double p2 = k2 * x2;
        const double both = p1 + p2;
        const double one = a1 * x1;
        e[i] = live2 ? both : (live1 ? one : x1);
    }
}

int launch_kcycle_sums1(hipStream_t s, int inner, const double* c1, const double* v1, const double* b, long long n, double* partials, const int* done)
{
    if (dot_reference_order()) {
        const double* u = inner ? v1 : c1;
        launch_dot_serial(s, u, v1, n, kcycle_region(partials, 0), done);
        launch_dot_serial(s, u, b, n, kcycle_region(partials, 1), done);
        return 1;
    }
    const int grid = grid_for(n, 1);
    if (inner) hipLaunchKernelGGL(kcycle_sums1_kernel<true>, dim3(grid), dim3(kBlock), 0, s, c1, v1, b, n, partials, done);
    else hipLaunchKernelGGL(kcycle_sums1_kernel<false>, dim3(grid), dim3(kBlock), 0, s, c1, v1, b, n, partials, done);
    return grid;
}

int launch_kcycle_sums2(hipStream_t s, int inner, const double* c2, const double* v2, const double* v1, const double* rr, long long n, double* partials, const int* done)
{
    if (dot_reference_order()) {
        const double* u = inner ? v2 : c2;
        launch_dot_serial(s, u, v1, n, kcycle_region(partials, 2), done);
        launch_dot_serial(s, u, v2, n, kcycle_region(partials, 3), done);
        launch_dot_serial(s, u, rr, n, kcycle_region(partials, 4), done);
        return 1;
    }
    const int grid = grid_for(n, 1);
    if (inner) hipLaunchKernelGGL(kcycle_sums2_kernel<true>, dim3(grid), dim3(kBlock), 0, s, c2, v2, v1, rr, n, partials, done);
    else hipLaunchKernelGGL(kcycle_sums2_kernel<false>, dim3(grid), dim3(kBlock), 0, s, c2, v2, v1, rr, n, partials, done);
    return grid;
}

void launch_kcycle_residual(hipStream_t s, const double* b, const double* v1, double* rr, long long n, const double* partials, int nPartials, const int* done)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(kcycle_residual_kernel, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, b, v1, rr, n, partials, nPartials, done);
}

void launch_kcycle_combine(hipStream_t s, const double* c1, const double* c2, double* e, long long n, const double* partials, int nPartials, const int* done)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(kcycle_combine_kernel, dim3(grid_for(n, 1)), dim3(kBlock), 0, s, c1, c2, e, n, partials, nPartials, done);
}

void preload_kernels_kcycle() { preload_code_object(reinterpret_cast<const void*>(&kcycle_combine_kernel)); }

} // namespace mgcg
