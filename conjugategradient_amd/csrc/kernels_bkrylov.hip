// Shared-subspace block CG for gfx950 (SolveBlockKrylov): k = 1..8 right-hand sides in ONE block Krylov space (O'Leary's block CG in
// Dubrulle's breakdown-free form BCGrQ).  SolveBlockEx (kernels_block.hip) runs k independent recurrences that share the matrix pass; here
// every column minimises over the union of the k Krylov spaces, so all of them converge in fewer iterations.
//
// Layout.  X and B are the caller's, column j at [j*n, (j+1)*n).  S (search block), Q (orthonormal residual block, holds W between the two
// passes) and T = A S live in the caller's p, r and Ap vectors, row-interleaved: v[i*k + j], the layout spmv_block_kernel gathers from.
// C, alpha, M, zeta and zeta^-1 are k x k matrices, row-major, in BkScalars.
//
// Method (include/MgcgGpu.h has the operation order).  Start: R = B - A X, R^T R = U^T U (Cholesky, U upper), Q = R U^-1, C = U, S = Q,
// rr0_j = sum_i C[i][j]^2.  Iteration:
//   1. T = A S ; G = S^T T                                (spmv_block_kernel<K, BEPI_GRAM>)
//   2. G = Ug^T Ug ; alpha = G^-1 ; M = alpha C           (bk_alpha_kernel)
//   3. X = X + S M ; W = Q - T alpha (over Q) ; H = W^T W (bk_pass1_kernel)
//   4. H = zeta^T zeta ; zeta^-1 ; C = zeta C ; rr_j = sum_i C[i][j]^2 ; decide_stop per column ; publish   (bk_zeta_kernel)
//   5. Q = W zeta^-1 ; S = Q + S zeta^T                   (bk_pass2_kernel)
// Q stays orthonormal and the columns' sizes travel in C: || r_j || = || C[:, j] ||, no extra sums.  Step 4 is a launch of its own (it is
// not folded into pass 2).
//
// Arithmetic.  Every product is rounded into a double of its own before the add that follows it (-ffp-contract=off); a sum over the k terms
// of a row starts with its first product and adds the others left to right, l = 0 .. k-1, structural zeros included.  The Gram matrices are
// tree sums of per-wavefront / per-workgroup partial sums added in a fixed order; under dot_order = 1 every entry is one serial left-to-right
// sum over the rows (bk_gram_serial_kernel, block_dot_serial_kernel's scheme) and the loop is a fixed sequence of IEEE operations.
//
// Stop flag.  The loop's flag is CgScalars::done of the handle (cg_drive polls it); every kernel returns at its first instruction once it is
// up.  A Cholesky pivot that is not finite and > 0 raises it with MGCG_NONFINITE for every column: in the start nothing has touched X, in
// step 2 X holds the previous iteration's update, in step 4 it holds this iteration's (a valid iterate whose residual norm is unknown).
#include "vec_passes.hpp"

namespace mgcg {

constexpr int kBkK = kBlockMaxK;
constexpr int kBkGram = kBkK * (kBkK + 1) / 2;        // entries of the upper triangle: 36

struct BkScalars {
    double C[kBkK * kBkK], alpha[kBkK * kBkK], M[kBkK * kBkK], zeta[kBkK * kBkK], zinv[kBkK * kBkK];
    double rr0[kBkK], residual[kBkK];
    int status[kBkK];
    int iteration;
    int failWhich, failPivot;                          // failWhich: 0 none, 1 R0^T R0, 2 S^T A S, 3 W^T W
    int pad;
};

bool Workspace::ensure_bkrylov()
{
    if (!gramPartials && !MGCG_HIP(hipMalloc((void**)&gramPartials, sizeof(double) * kBkGram * (size_t)kMaxPartials))) return false;
    if (!bkScalars) {
        if (!MGCG_HIP(hipMalloc((void**)&bkScalars, sizeof(BkScalars)))) return false;
        if (!MGCG_HIP(hipMemset(bkScalars, 0, sizeof(BkScalars)))) return false;
    }
    return true;
}

// ------------------------------------------------------------------ k x k algebra (one thread, fp64, plain sqrt and /)
// Upper triangle of the k x k Gram matrix from its partial sums, by the whole workgroup: entry e's n partials at partials + e * kMaxPartials.
__device__ __forceinline__ void bk_reduce_gram(const double* __restrict__ partials, int n, int k, double (*s_red)[4], double* s_g)
{
    int e = 0;
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b, ++e) {
            const double v = reduce_partials_block(partials + (long long)e * kMaxPartials, n, s_red[e], 0);
            if (threadIdx.x == 0) s_g[a * kBkK + b] = v;
        }
    __syncthreads();
}

// G = U^T U from G's upper triangle, U upper triangular (its lower triangle is set to 0).  Returns -1, or the index of the first pivot
// that is not finite and > 0.
__device__ int bk_cholesky(const double* G, double* U, int k)
{
    for (int i = 0; i < k; ++i) {
        double d = G[i * kBkK + i];
        for (int l = 0; l < i; ++l) { const double t = U[l * kBkK + i] * U[l * kBkK + i]; d = d - t; }
        if (!(d > 0.0 && d <= 1.79e308)) return i;
        const double u = sqrt(d);
        U[i * kBkK + i] = u;
        for (int j = i + 1; j < k; ++j) {
            double s = G[i * kBkK + j];
            for (int l = 0; l < i; ++l) { const double t = U[l * kBkK + i] * U[l * kBkK + j]; s = s - t; }
            U[i * kBkK + j] = s / u;
            U[j * kBkK + i] = 0.0;
        }
    }
    return -1;
}

// V = U^-1 for upper triangular U (V upper triangular, its lower triangle 0)
__device__ void bk_invert_upper(const double* U, double* V, int k)
{
    for (int j = 0; j < k; ++j) {
        for (int i = j + 1; i < k; ++i) V[i * kBkK + j] = 0.0;
        V[j * kBkK + j] = 1.0 / U[j * kBkK + j];
        for (int i = j - 1; i >= 0; --i) {
            double s = U[i * kBkK + i + 1] * V[(i + 1) * kBkK + j];
            for (int l = i + 2; l <= j; ++l) { const double t = U[i * kBkK + l] * V[l * kBkK + j]; s = s + t; }
            V[i * kBkK + j] = (-s) / U[i * kBkK + i];
        }
    }
}

// P = A B (k x k, full sums l = 0 .. k-1, the first product then the adds)
__device__ void bk_matmul(const double* A, const double* B, double* P, int k)
{
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            double s = A[a * kBkK] * B[b];
            for (int l = 1; l < k; ++l) { const double t = A[a * kBkK + l] * B[l * kBkK + b]; s = s + t; }
            P[a * kBkK + b] = s;
        }
}

__device__ double bk_column_norm2(const double* C, int j, int k)
{
    double s = C[j] * C[j];
    for (int i = 1; i < k; ++i) { const double t = C[i * kBkK + j] * C[i * kBkK + j]; s = s + t; }
    return s;
}

__device__ void bk_fail(BkScalars* bk, CgScalars* sc, int k, int which, int pivot)
{
    for (int j = 0; j < k; ++j) bk->status[j] = MGCG_NONFINITE;
    bk->failWhich = which; bk->failPivot = pivot;
    sc->status = MGCG_NONFINITE;
    sc->done = 1;
}

// Start: R^T R = U^T U ; C = U ; zinv = U^-1 (pass 2's start form makes Q = R U^-1 of it) ; rr0
__global__ __launch_bounds__(kBlock) void bk_start_kernel(BkScalars* bk, CgScalars* sc, const double* __restrict__ partials, int n, int k)
{
    __shared__ double s_red[kBkGram][4];
    __shared__ double s_g[kBkK * kBkK];
    if (sc->done != 0) return;
    bk_reduce_gram(partials, n, k, s_red, s_g);
    if (threadIdx.x != 0) return;
    bk->iteration = 0; bk->failWhich = 0; bk->failPivot = -1;
    for (int j = 0; j < kBkK; ++j) { bk->status[j] = MGCG_OK; bk->residual[j] = 0.0; bk->rr0[j] = 0.0; }
    const int bad = bk_cholesky(s_g, bk->C, k);
    if (bad >= 0) { bk_fail(bk, sc, k, 1, bad); return; }
    bk_invert_upper(bk->C, bk->zinv, k);
    for (int j = 0; j < k; ++j) bk->rr0[j] = bk_column_norm2(bk->C, j, k);
}

// Step 2: G = Ug^T Ug ; V = Ug^-1 ; alpha = V V^T ; M = alpha C
__global__ __launch_bounds__(kBlock) void bk_alpha_kernel(BkScalars* bk, CgScalars* sc, const double* __restrict__ partials, int n, int k)
{
    __shared__ double s_red[kBkGram][4];
    __shared__ double s_g[kBkK * kBkK];
    __shared__ double s_u[kBkK * kBkK], s_v[kBkK * kBkK];
    if (sc->done != 0) return;
    bk_reduce_gram(partials, n, k, s_red, s_g);
    if (threadIdx.x != 0) return;
    const int bad = bk_cholesky(s_g, s_u, k);
    if (bad >= 0) { bk_fail(bk, sc, k, 2, bad); return; }
    bk_invert_upper(s_u, s_v, k);
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b) {                  // alpha[a][b] = sum over l = b .. k-1 of V[a][l] V[b][l], mirrored
            double s = s_v[a * kBkK + b] * s_v[b * kBkK + b];
            for (int l = b + 1; l < k; ++l) { const double t = s_v[a * kBkK + l] * s_v[b * kBkK + l]; s = s + t; }
            bk->alpha[a * kBkK + b] = s; bk->alpha[b * kBkK + a] = s;
        }
    bk_matmul(bk->alpha, bk->C, bk->M, k);
}

// Step 4: H = zeta^T zeta ; zinv ; C = zeta C ; rr_j ; the stop decision of the iteration per column ; publish
__global__ __launch_bounds__(kBlock) void bk_zeta_kernel(BkScalars* bk, CgScalars* sc, const double* __restrict__ partials, int n, int k, FinalizeArgs f)
{
    __shared__ double s_red[kBkGram][4];
    __shared__ double s_g[kBkK * kBkK];
    __shared__ double s_c[kBkK * kBkK];
    if (sc->done != 0) return;
    bk_reduce_gram(partials, n, k, s_red, s_g);
    if (threadIdx.x != 0) return;
    const int bad = bk_cholesky(s_g, bk->zeta, k);
    if (bad >= 0) { bk_fail(bk, sc, k, 3, bad); return; }
    bk_invert_upper(bk->zeta, bk->zinv, k);
    bk_matmul(bk->zeta, bk->C, s_c, k);
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) bk->C[a * kBkK + b] = s_c[a * kBkK + b];
    const int it = bk->iteration;
    bool goOn = false;
    int worst = MGCG_OK;
    for (int j = 0; j < k; ++j) {
        const double rr = bk_column_norm2(s_c, j, k);
        const StopDecision d = decide_stop(f, rr, 0.0, bk->rr0[j], it);
        if (f.trace != nullptr && it < f.traceCap) f.trace[(long long)j * f.traceCap + it] = d.shown;
        bk->residual[j] = d.res; bk->status[j] = d.status;
        goOn = goOn || !d.stop;
        if (d.status == MGCG_NONFINITE) worst = MGCG_NONFINITE;
        else if (d.status == MGCG_MAXIT_EXCEEDED && worst == MGCG_OK) worst = MGCG_MAXIT_EXCEEDED;
    }
    if (goOn) bk->iteration = it + 1;
    else { sc->status = worst; sc->done = 1; }
}

// ------------------------------------------------------------------ rows of the blocks
// R rows (1, or 2 with 16-byte accesses) of an interleaved block from row i: 2 K doubles from an even row are 16-byte aligned for every K
template <int K, int R, bool NTV>
__device__ __forceinline__ void bk_load_rows(const double* __restrict__ p, long long i, double (&v)[R][K])
{
    if constexpr (R == 2) {
        const d2* q = (const d2*)(p + i * K);
#pragma unroll
        for (int f = 0; f < K; ++f) { const d2 t = ldv<NTV>(q + f); v[(2 * f) / K][(2 * f) % K] = t.x; v[(2 * f + 1) / K][(2 * f + 1) % K] = t.y; }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[0][j] = p[i * K + j];
    }
}
template <int K, int R, bool NTV>
__device__ __forceinline__ void bk_store_rows(double* __restrict__ p, long long i, const double (&v)[R][K])
{
    if constexpr (R == 2) {
        d2* q = (d2*)(p + i * K);
#pragma unroll
        for (int f = 0; f < K; ++f) { d2 t; t.x = v[(2 * f) / K][(2 * f) % K]; t.y = v[(2 * f + 1) / K][(2 * f + 1) % K]; stv<NTV>(t, q + f); }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) p[i * K + j] = v[0][j];
    }
}

// out[r][j] = sum over l of in[r][l] * m[l][j]: the first product, then the adds, left to right (m: a k x k matrix in LDS, row stride kBkK)
template <int K, int R>
__device__ __forceinline__ void bk_rows_times(const double (&in)[R][K], const double* m, double (&out)[R][K])
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) out[r][j] = in[r][0] * m[j];
#pragma unroll
        for (int l = 1; l < K; ++l) {
            const double c = m[l * kBkK + j];
#pragma unroll
            for (int r = 0; r < R; ++r) { const double t = in[r][l] * c; out[r][j] = out[r][j] + t; }
        }
    }
}

// the k x k matrices of a pass into LDS (broadcast reads from there)
__device__ __forceinline__ void bk_stage(const double* __restrict__ a, const double* __restrict__ b, double* s_a, double* s_b)
{
    if (threadIdx.x < kBkK * kBkK) { s_a[threadIdx.x] = a[threadIdx.x]; if (b != nullptr) s_b[threadIdx.x] = b[threadIdx.x]; }
    __syncthreads();
}

// per-workgroup sums of the K (K + 1) / 2 accumulators -> partials[e * kMaxPartials + blockIdx.x]
template <int K>
__device__ __forceinline__ void bk_gram_out(double (&h)[K * (K + 1) / 2], double* __restrict__ partials)
{
    constexpr int nE = K * (K + 1) / 2;
    __shared__ double s_sum[nE][4];
#pragma unroll
    for (int e = 0; e < nE; ++e) {
        const double t = wave_sum_b(h[e]);
        if ((threadIdx.x & 63) == 0) s_sum[e][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < nE) {
        const int e = threadIdx.x;
        partials[(long long)e * kMaxPartials + blockIdx.x] = (s_sum[e][0] + s_sum[e][1]) + (s_sum[e][2] + s_sum[e][3]);
    }
}

template <int K, int R>
__device__ __forceinline__ void bk_gram_add(const double (&w)[R][K], double (&h)[K * (K + 1) / 2])
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < K; ++a) {
#pragma unroll
            for (int b = a; b < K; ++b) { const double t = w[r][a] * w[r][b]; h[e] += t; ++e; }
        }
    }
}

// ------------------------------------------------------------------ start
// S = interleave(X)
template <int K>
__global__ __launch_bounds__(kBlock) void bk_interleave_kernel(const int* done, double* __restrict__ S, const double* __restrict__ X, long long n)
{
    if (*done != 0) return;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; ++j) S[i * K + j] = X[j * n + i];
    }
}

// R = B - T into Q (interleaved) ; partial sums of the upper triangle of R^T R
template <int K>
__global__ __launch_bounds__(kBlock) void bk_residual_kernel(const int* done, double* __restrict__ Q, const double* __restrict__ T, const double* __restrict__ B, long long n,
                                                             double* __restrict__ partials)
{
    if (*done != 0) return;
    double h[K * (K + 1) / 2];
#pragma unroll
    for (int e = 0; e < K * (K + 1) / 2; ++e) h[e] = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double r[1][K];
#pragma unroll
        for (int j = 0; j < K; ++j) { r[0][j] = B[j * n + i] - T[i * K + j]; Q[i * K + j] = r[0][j]; }
        bk_gram_add<K, 1>(r, h);
    }
    bk_gram_out<K>(h, partials);
}

// ------------------------------------------------------------------ pass 1: X = X + S M ; W = Q - T alpha (over Q) ; partial sums of W^T W
template <int K, int R, bool NTV>
__device__ __forceinline__ void bk_pass1_rows(long long i, long long n, const double* s_m, const double* s_alpha, double* __restrict__ X, const double* __restrict__ S,
                                              const double* __restrict__ T, double* __restrict__ Q, double (&h)[K * (K + 1) / 2])
{
    double sv[R][K], tv[R][K], qv[R][K], u[R][K];
    bk_load_rows<K, R, NTV>(S, i, sv);
    bk_load_rows<K, R, NTV>(T, i, tv);
    bk_load_rows<K, R, NTV>(Q, i, qv);
    bk_rows_times<K, R>(sv, s_m, u);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if constexpr (R == 2) {
            d2* xp = (d2*)(X + j * n + i);
            d2 xv = ldv<NTV>(xp);
            xv.x = xv.x + u[0][j]; xv.y = xv.y + u[1][j];
            stv<NTV>(xv, xp);
        } else {
            X[j * n + i] = X[j * n + i] + u[0][j];
        }
    }
    bk_rows_times<K, R>(tv, s_alpha, u);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < K; ++j) qv[r][j] = qv[r][j] - u[r][j];
    }
    bk_store_rows<K, R, NTV>(Q, i, qv);
    bk_gram_add<K, R>(qv, h);
}

template <int K, bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void bk_pass1_kernel(const int* done, const BkScalars* __restrict__ bk, double* __restrict__ X, const double* __restrict__ S,
                                                          const double* __restrict__ T, double* __restrict__ Q, long long n, double* __restrict__ partials)
{
    __shared__ double s_m[kBkK * kBkK], s_alpha[kBkK * kBkK];
    if (*done != 0) return;
    bk_stage(bk->M, bk->alpha, s_m, s_alpha);
    double h[K * (K + 1) / 2];
#pragma unroll
    for (int e = 0; e < K * (K + 1) / 2; ++e) h[e] = 0.0;
    grid_stride<V2>(n, [&](long long i) { bk_pass1_rows<K, 2, NTV>(i, n, s_m, s_alpha, X, S, T, Q, h); },
                    [&](long long i) { bk_pass1_rows<K, 1, false>(i, n, s_m, s_alpha, X, S, T, Q, h); });
    bk_gram_out<K>(h, partials);
}

// ------------------------------------------------------------------ pass 2: Q = W zeta^-1 ; S = Q + S zeta^T   (START: Q = R U^-1 ; S = Q)
template <int K, int R, bool NTV, bool START>
__device__ __forceinline__ void bk_pass2_rows(long long i, const double* s_zinv, const double* s_zetaT, double* __restrict__ S, double* __restrict__ Q)
{
    double wv[R][K], qv[R][K];
    bk_load_rows<K, R, NTV>(Q, i, wv);
    bk_rows_times<K, R>(wv, s_zinv, qv);
    bk_store_rows<K, R, NTV>(Q, i, qv);
    if constexpr (!START) {
        double sv[R][K], u[R][K];
        bk_load_rows<K, R, NTV>(S, i, sv);
        bk_rows_times<K, R>(sv, s_zetaT, u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int j = 0; j < K; ++j) qv[r][j] = qv[r][j] + u[r][j];
        }
    }
    bk_store_rows<K, R, NTV>(S, i, qv);
}

template <int K, bool V2, bool NTV, bool START>
__global__ __launch_bounds__(kBlock) void bk_pass2_kernel(const int* done, const BkScalars* __restrict__ bk, double* __restrict__ S, double* __restrict__ Q, long long n)
{
    __shared__ double s_zinv[kBkK * kBkK], s_zetaT[kBkK * kBkK];
    if (*done != 0) return;
    if (threadIdx.x < kBkK * kBkK) {
        s_zinv[threadIdx.x] = bk->zinv[threadIdx.x];
        if constexpr (!START) s_zetaT[threadIdx.x] = bk->zeta[(threadIdx.x % kBkK) * kBkK + threadIdx.x / kBkK];      // zeta^T[l][j] = zeta[j][l]
    }
    __syncthreads();
    grid_stride<V2>(n, [&](long long i) { bk_pass2_rows<K, 2, NTV, START>(i, s_zinv, s_zetaT, S, Q); },
                    [&](long long i) { bk_pass2_rows<K, 1, false, START>(i, s_zinv, s_zetaT, S, Q); });
}

// ------------------------------------------------------------------ validation mode (knob dot_order): serial Gram entries
// Workgroup e = entry (a, b), a <= b: sum over the rows i of x[i*k + a] * y[i*k + b], rounded products added strictly left to right
// (block_dot_serial_kernel's scheme: waves 1-3 stage the products of the next batch in LDS, lane 0 of wave 0 adds the current one).
constexpr int kBkSerialBatch = 2048;
__global__ __launch_bounds__(kBlock) void bk_gram_serial_kernel(const int* done, const double* __restrict__ x, const double* __restrict__ y, long long n, int k,
                                                                double* __restrict__ out)
{
    __shared__ double s_prod[2][kBkSerialBatch];
    if (*done != 0) return;
    int a = 0, b = (int)blockIdx.x;
    while (b >= k - a) { b -= k - a; ++a; }
    b += a;
    const double* xc = x + a;
    const double* yc = y + b;
    const int tid = threadIdx.x;
    const long long nBatches = (n + kBkSerialBatch - 1) / kBkSerialBatch;
    auto fill = [&](int buf, long long bt) {
        const long long base = bt * kBkSerialBatch;
        for (int q = tid - kWave; q < kBkSerialBatch; q += kBlock - kWave) {
            const long long i = base + q;
            double t = 0.0;
            if (i < n) t = xc[i * k] * yc[i * k];
            s_prod[buf][q] = t;
        }
    };
    if (tid >= kWave) fill(0, 0);
    __syncthreads();
    double acc = 0.0;
    for (long long bt = 0; bt < nBatches; ++bt) {
        if (tid >= kWave) { if (bt + 1 < nBatches) fill((int)((bt + 1) & 1), bt + 1); }
        else if (tid == 0) {
            const double* q = s_prod[bt & 1];
#pragma unroll 16
            for (int i = 0; i < kBkSerialBatch; ++i) acc += q[i];
        }
        __syncthreads();
    }
    if (tid == 0) out[(long long)blockIdx.x * kMaxPartials] = acc;
}

// ------------------------------------------------------------------ launches
static int bk_gram_serial(hipStream_t s, const int* done, const double* x, const double* y, long long n, int k, double* partials)
{
    hipLaunchKernelGGL(bk_gram_serial_kernel, dim3(k * (k + 1) / 2), dim3(kBlock), 0, s, done, x, y, n, k, partials);
    return 1;
}

// 16-byte accesses: two rows per lane; every column of X must then start on a 16-byte boundary (an even row count, or one column)
template <int K>
static bool bk_v2(const BkRun& R) { return al16(R.X) && al16(R.S) && al16(R.T) && al16(R.Q) && (K == 1 || (R.n & 1) == 0); }

template <int K>
static bool bk_enqueue_start_k(const BkRun& R)
{
    hipStream_t s = R.ws->stream;
    const int* done = &R.ws->scalars->done;
    double* P = R.ws->gramPartials;
    const int g = grid_for(R.n, 1);
    hipLaunchKernelGGL((bk_interleave_kernel<K>), dim3(g), dim3(kBlock), 0, s, done, R.S, (const double*)R.X, R.n);
    (void)launch_spmv_block_gram(s, K, R.elements, R.rowOffsets, R.columnIndeces, R.S, R.T, R.n, P, done);       // T = A X (its sums are not used)
    hipLaunchKernelGGL((bk_residual_kernel<K>), dim3(g), dim3(kBlock), 0, s, done, R.Q, (const double*)R.T, R.B, R.n, P);
    int nP = g;
    if (dot_reference_order()) nP = bk_gram_serial(s, done, R.Q, R.Q, R.n, K, P);
    hipLaunchKernelGGL(bk_start_kernel, dim3(1), dim3(kBlock), 0, s, R.ws->bkScalars, R.ws->scalars, (const double*)P, nP, K);
    with_v2_nt(bk_v2<K>(R), vec_nt(R.n), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((bk_pass2_kernel<K, V2.value, NTV.value, true>), dim3(grid_for(R.n, V2.value ? 2 : 1)), dim3(kBlock), 0, s, done,
                           (const BkScalars*)R.ws->bkScalars, R.S, R.Q, R.n);
    });
    return MGCG_HIP(hipGetLastError());
}

template <int K>
static bool bk_enqueue_iteration_k(const BkRun& R, const FinalizeArgs& f)
{
    hipStream_t s = R.ws->stream;
    CgScalars* sc = R.ws->scalars;
    const int* done = &sc->done;
    BkScalars* bk = R.ws->bkScalars;
    double* P = R.ws->gramPartials;
    const bool ref = dot_reference_order();
    int nG = launch_spmv_block_gram(s, K, R.elements, R.rowOffsets, R.columnIndeces, R.S, R.T, R.n, P, done);    // 1. T = A S ; S^T T
    if (ref) nG = bk_gram_serial(s, done, R.S, R.T, R.n, K, P);
    hipLaunchKernelGGL(bk_alpha_kernel, dim3(1), dim3(kBlock), 0, s, bk, sc, (const double*)P, nG, K);         // 2. alpha, M
    int nH = 0;
    with_v2_nt(bk_v2<K>(R), vec_nt(R.n), [&](auto V2, auto NTV) {
        nH = grid_for(R.n, V2.value ? 2 : 1);
        hipLaunchKernelGGL((bk_pass1_kernel<K, V2.value, NTV.value>), dim3(nH), dim3(kBlock), 0, s, done, (const BkScalars*)bk, R.X, (const double*)R.S,
                           (const double*)R.T, R.Q, R.n, P);                                                    // 3. X, W ; W^T W
    });
    if (ref) nH = bk_gram_serial(s, done, R.Q, R.Q, R.n, K, P);
    hipLaunchKernelGGL(bk_zeta_kernel, dim3(1), dim3(kBlock), 0, s, bk, sc, (const double*)P, nH, K, f);       // 4. zeta, C, the stop decision
    with_v2_nt(bk_v2<K>(R), vec_nt(R.n), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((bk_pass2_kernel<K, V2.value, NTV.value, false>), dim3(grid_for(R.n, V2.value ? 2 : 1)), dim3(kBlock), 0, s, done,
                           (const BkScalars*)bk, R.S, R.Q, R.n);                                               // 5. Q, S
    });
    return MGCG_HIP(hipGetLastError());
}

bool bk_enqueue_start(const BkRun& R) { return dispatch_k(R.k, [&](auto K) { return bk_enqueue_start_k<K.value>(R); }); }
bool bk_enqueue_iteration(const BkRun& R, const FinalizeArgs& f) { return dispatch_k(R.k, [&](auto K) { return bk_enqueue_iteration_k<K.value>(R, f); }); }

bool bk_read_results(Workspace* ws, int k, BkResult* out)
{
    BkScalars h;
    if (!MGCG_HIP(hipMemcpy(&h, ws->bkScalars, sizeof(h), hipMemcpyDeviceToHost))) return false;
    out->iteration = h.iteration; out->failWhich = h.failWhich; out->failPivot = h.failPivot;
    for (int j = 0; j < k; ++j) { out->residual[j] = h.residual[j]; out->status[j] = h.status[j]; }
    return true;
}

void preload_kernels_bkrylov() { preload_code_object(reinterpret_cast<const void*>(&bk_start_kernel)); }

} // namespace mgcg
