// LOBPCG for gfx950 (MgcgSolveLobpcg, MgcgSolveLobpcgMg): the k = 1..8 lowest (or highest) eigenpairs of a symmetric CSR matrix by Knyazev's
// locally optimal block preconditioned CG.  include/MgcgGpu.h has the method as computed; this file has the passes and the dense step.
//
// Layout.  Every block is column-major: X is the caller's, column j at j * n; AX, W, AW, P, AP and R are the six blocks of the work vector,
// column j of each at j * ld (ld = n rounded up to even).  The passes take lists of column addresses (LobCols), so S = [X W P] and
// AS = [AX AW AP] are never copied together.  The product is CsrMVBlock's k-column kernel on operands ld apart (launch_spmv_block_plain).
//
// The four kinds of launch.
//   residual  lob_residual_kernel: R = AX - X diag(theta), the k column sums of squares, and W = R or W = dinv o R, in one read.
//   Gram      lob_gram_kernel: entries (a, b) = sum_i L_a[i] R_b[i] of a product of two column lists.  The triangle is cut by K x K tiles of
//             column groups over blockIdx.y (K = k: the groups are X, W, P), K^2 accumulators per lane, so G_B = S^T S and G_A = S^T AS are
//             two launches of six tiles each at m = 3k; a tile below the diagonal returns at once.  Per-workgroup partial sums in a fixed
//             order (wavefront tree, four wavefronts, then the workgroups left to right in the dense step).  X^T W (full) and W^T W
//             (upper) are the same kernel on one tile.  Under dot_order = 1 lob_gram_serial_kernel forms every entry by one workgroup as
//             one serial left-to-right sum over the rows (bk_gram_serial_kernel's scheme).
//   combine   lob_combine_kernel: row local; a lane reads its row's MI values of a column list and writes MO columns in place from an
//             MI x MO coefficient block staged in LDS: out_c = sum over l = l0_c .. mUse-1 of in_l * C[l][c], the first product, then the
//             adds left to right.  X Ui, X Z, W - X (X^T W), W T and the body's X, AX, P, AP are this kernel with other coefficients;
//             blockIdx.y chooses the family (S or AS).  mUse is read from the device: the dense step decides there whether P takes part.
//   dense     one workgroup: the partial sums, the dense products and the Jacobi rotations (a row of H and of Z per lane) are the workgroup's
//             work in LDS, the factorisations, the sort, the coefficients and the stop decision one lane's.  No value crosses to the host inside the loop except the stop flag.
//
// Arithmetic.  Every product is rounded into a double of its own before the add that follows it (-ffp-contract=off); every sum over a block
// index starts with its first product and adds the others left to right, structural zeros included.  Under dot_order = 1 the loop is a
// fixed sequence of IEEE operations (tests/test_lobpcg_host.py restates it in numpy).
#include "vec_passes.hpp"

namespace mgcg {

constexpr int kLobK = kBlockMaxK;
constexpr int kLobM = 3 * kLobK;                      // columns of the basis [X W P]: 24
constexpr int kLobP = 128;                            // workgroups of a Gram pass = partial sums per entry
constexpr int kLobRegion = kLobM * kLobM * kLobP;     // one region of partial sums: entry (a, b) at (a * kLobM + b) * kLobP
constexpr int kLobSweeps = 30;
constexpr double kLobEps = 1.1102230246251565e-16;    // 2^-53
constexpr double kLobDropP = 9.5367431640625e-07;     // 2^-20: P is dropped when a pivot of the 3k basis keeps no more than this share of its column

struct LobCols { const double* c[kLobM]; };
struct LobOut { double* c[2 * kLobK]; };

struct LobScalars {
    double CC[kLobM * 2 * kLobK];                     // the coefficients of the next combine pass, row l at l * 2 kLobK
    double theta[kLobK], residual[kLobK], trueResidual[kLobK];
    int status[kLobK];
    int iteration, restarts, skip, mUse;
    int failWhich, failPivot;
    int zero, pad;                                    // zero: a stop flag that is never up (the close runs behind a raised flag)
};

bool Workspace::ensure_lobpcg()
{
    if (!lobPartials && !MGCG_HIP(hipMalloc((void**)&lobPartials, sizeof(double) * 3 * (size_t)kLobRegion))) return false;
    if (!lobScalars) {
        if (!MGCG_HIP(hipMalloc((void**)&lobScalars, sizeof(LobScalars)))) return false;
        if (!MGCG_HIP(hipMemset(lobScalars, 0, sizeof(LobScalars)))) return false;
    }
    return true;
}

// ------------------------------------------------------------------ the dense algebra (one lane, fp64, plain sqrt and /, row stride kLobM)
// G = U^T U from G's upper triangle (bk_cholesky's order of operations); -1, or the first pivot that is not finite and > 0 -- with tau > 0:
// and > tau * G_ii, the share of the column's own square that is left once the columns before it are taken out
__device__ int lob_cholesky(const double* G, double* U, int m, double tau = 0.0)
{
    for (int i = 0; i < m; ++i) {
        double d = G[i * kLobM + i];
        for (int l = 0; l < i; ++l) { const double t = U[l * kLobM + i] * U[l * kLobM + i]; d = d - t; }
        const double floor = tau * G[i * kLobM + i];
        if (!(positive_finite(d) && d > floor)) return i;
        const double u = sqrt(d);
        U[i * kLobM + i] = u;
        for (int j = i + 1; j < m; ++j) {
            double s = G[i * kLobM + j];
            for (int l = 0; l < i; ++l) { const double t = U[l * kLobM + i] * U[l * kLobM + j]; s = s - t; }
            U[i * kLobM + j] = s / u;
            U[j * kLobM + i] = 0.0;
        }
    }
    return -1;
}
// V = U^-1, upper triangular (bk_invert_upper's order)
__device__ void lob_invert_upper(const double* U, double* V, int m)
{
    for (int j = 0; j < m; ++j) {
        for (int i = j + 1; i < m; ++i) V[i * kLobM + j] = 0.0;
        V[j * kLobM + j] = 1.0 / U[j * kLobM + j];
        for (int i = j - 1; i >= 0; --i) {
            double s = U[i * kLobM + i + 1] * V[(i + 1) * kLobM + j];
            for (int l = i + 2; l <= j; ++l) { const double t = U[i * kLobM + l] * V[l * kLobM + j]; s = s + t; }
            V[i * kLobM + j] = (-s) / U[i * kLobM + i];
        }
    }
}
// P = A B, A ra x inner (TA: its transpose is stored), B inner x cb: full sums l = 0 .. inner-1, the first product then the adds.  By the whole
// workgroup, an entry per lane; a barrier follows.
template <bool TA>
__device__ void lob_mm(const double* A, const double* B, double* P, int ra, int inner, int cb)
{
    for (int e = threadIdx.x; e < ra * cb; e += kBlock) {
        const int a = e / cb, b = e % cb;
        double s = (TA ? A[a] : A[a * kLobM]) * B[b];
        for (int l = 1; l < inner; ++l) { const double t = (TA ? A[l * kLobM + a] : A[a * kLobM + l]) * B[l * kLobM + b]; s = s + t; }
        P[a * kLobM + b] = s;
    }
    __syncthreads();
}
__device__ void lob_mirror(double* G, int m)
{
    for (int a = 0; a < m; ++a)
        for (int b = a + 1; b < m; ++b) G[b * kLobM + a] = G[a * kLobM + b];
}

// H = V diag(w) V^T by cyclic Jacobi rotations (include/MgcgGpu.h states the scheme): H symmetric and full on entry, its diagonal holds w on
// return; V's columns are the eigenvectors.  By the whole workgroup: every lane forms the rotation from the same values in LDS, lane r
// updates row r of H and of V, lane 0 the pivot block; the operations of every entry are those of a serial loop.
__device__ void lob_jacobi(double* H, double* V, int m)
{
    const int r = threadIdx.x;
    for (int e = r; e < m * m; e += kBlock) V[(e / m) * kLobM + e % m] = e / m == e % m ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < kLobSweeps; ++sweep) {
        int rotated = 0;
        for (int p = 0; p + 1 < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double hpq = H[p * kLobM + q], hpp = H[p * kLobM + p], hqq = H[q * kLobM + q];
                __syncthreads();                       // every lane has the pivot block before a lane overwrites it
                if (!(fabs(hpq) > kLobEps * (fabs(hpp) + fabs(hqq)))) continue;
                const double tau = (hqq - hpp) / (2.0 * hpq);
                const double tt = tau * tau;
                double t = 1.0 / (fabs(tau) + sqrt(1.0 + tt));
                if (tau < 0.0) t = -t;
                const double t2 = t * t;
                const double c = 1.0 / sqrt(1.0 + t2), s = t * c;
                if (r < m) {
                    if (r != p && r != q) {
                        const double x = H[r * kLobM + p], y = H[r * kLobM + q];
                        const double cx = c * x, sy = s * y, sx = s * x, cy = c * y;
                        const double np = cx - sy, nq = sx + cy;
                        H[r * kLobM + p] = np; H[p * kLobM + r] = np;
                        H[r * kLobM + q] = nq; H[q * kLobM + r] = nq;
                    }
                    const double x = V[r * kLobM + p], y = V[r * kLobM + q];
                    const double cx = c * x, sy = s * y, sx = s * x, cy = c * y;
                    V[r * kLobM + p] = cx - sy; V[r * kLobM + q] = sx + cy;
                }
                if (r == 0) {
                    const double tp = t * hpq;
                    H[p * kLobM + p] = hpp - tp; H[q * kLobM + q] = hqq + tp;
                    H[p * kLobM + q] = 0.0; H[q * kLobM + p] = 0.0;
                }
                ++rotated;
                __syncthreads();                       // the rotation is complete before the next pair is read
            }
        if (rotated == 0) break;
    }
}
// perm: the indices of the diagonal of H in ascending order (descending with `largest`), equal values in index order (a stable insertion sort)
__device__ void lob_sort(const double* H, int m, int largest, int* perm)
{
    for (int i = 0; i < m; ++i) {
        const double wi = H[i * kLobM + i];
        int j = i;
        while (j > 0) {
            const double wj = H[perm[j - 1] * kLobM + perm[j - 1]];
            if (largest ? wi > wj : wi < wj) { perm[j] = perm[j - 1]; --j; } else break;
        }
        perm[j] = i;
    }
}

// The entries of a Gram matrix from their partial sums, by the whole workgroup, the workgroups' sums left to right: mode 0 every entry of
// mL x mR, 1 the upper triangle, 2 the diagonal.
__device__ void lob_reduce(const double* __restrict__ partials, int nP, int mL, int mR, int mode, double* G)
{
    for (int e = threadIdx.x; e < mL * mR; e += kBlock) {
        const int a = e / mR, b = e % mR;
        if ((mode == 1 && a > b) || (mode == 2 && a != b)) continue;
        const double* p = partials + (long long)(a * kLobM + b) * kLobP;
        double s = p[0];
        for (int i = 1; i < nP; ++i) s += p[i];
        G[a * kLobM + b] = s;
    }
    __syncthreads();
}

__device__ void lob_fail(LobScalars* lb, CgScalars* sc, int k, int which, int pivot)
{
    for (int j = 0; j < k; ++j) lb->status[j] = MGCG_NONFINITE;
    lb->failWhich = which; lb->failPivot = pivot;
    sc->status = MGCG_NONFINITE;
    sc->done = 1;
}

// ------------------------------------------------------------------ the dense launches
// Start, 1: X^T X = U^T U ; CC = U^-1 (the combine pass makes X = X U^-1, AX = AX U^-1 of it)
__global__ __launch_bounds__(kBlock) void lob_start_kernel(LobScalars* lb, CgScalars* sc, const double* __restrict__ pB, int nP, int k)
{
    __shared__ double s_g[kLobM * kLobM], s_u[kLobM * kLobM], s_v[kLobM * kLobM];
    if (sc->done != 0) return;
    lob_reduce(pB, nP, k, k, 1, s_g);
    if (threadIdx.x != 0) return;
    lb->iteration = 0; lb->restarts = 0; lb->skip = 0; lb->mUse = k; lb->failWhich = 0; lb->failPivot = -1; lb->zero = 0;
    for (int j = 0; j < kLobK; ++j) { lb->status[j] = MGCG_OK; lb->residual[j] = 0.0; lb->theta[j] = 0.0; lb->trueResidual[j] = 0.0; }
    const int bad = lob_cholesky(s_g, s_u, k);
    if (bad >= 0) { lob_fail(lb, sc, k, 1, bad); return; }
    lob_invert_upper(s_u, s_v, k);
    for (int l = 0; l < k; ++l)
        for (int j = 0; j < k; ++j) lb->CC[l * 2 * kLobK + j] = s_v[l * kLobM + j];
}

// Start, 2: H = X^T AX = Z diag(theta) Z^T ; CC = Z in the order of theta
__global__ __launch_bounds__(kBlock) void lob_ritz0_kernel(LobScalars* lb, CgScalars* sc, const double* __restrict__ pA, int nP, int k, int largest)
{
    __shared__ double s_h[kLobM * kLobM], s_v[kLobM * kLobM];
    __shared__ int s_perm[kLobM];
    if (sc->done != 0) return;
    lob_reduce(pA, nP, k, k, 1, s_h);
    if (threadIdx.x == 0) lob_mirror(s_h, k);
    __syncthreads();
    lob_jacobi(s_h, s_v, k);
    if (threadIdx.x != 0) return;
    lob_sort(s_h, k, largest, s_perm);
    for (int j = 0; j < k; ++j) {
        const double w = s_h[s_perm[j] * kLobM + s_perm[j]];
        if (!finite_value(w)) { lob_fail(lb, sc, k, 5, j); return; }
    }
    for (int j = 0; j < k; ++j) {
        lb->theta[j] = s_h[s_perm[j] * kLobM + s_perm[j]];
        for (int l = 0; l < k; ++l) lb->CC[l * 2 * kLobK + j] = s_v[l * kLobM + s_perm[j]];
    }
}

// Body, 1: rn_j = sqrt(R_j . R_j), the stop decision of body `iteration`, the trace ; CC = X^T W
__global__ __launch_bounds__(kBlock) void lob_judge_kernel(LobScalars* lb, CgScalars* sc, const double* __restrict__ pR, int nR, const double* __restrict__ pB, int nB,
                                                           int k, double tol, int relative, int minIt, int maxIt, double* trace, int traceCap)
{
    __shared__ double s_r[kLobM * kLobM], s_g[kLobM * kLobM];
    if (sc->done != 0) return;
    lob_reduce(pR, nR, k, k, 2, s_r);
    lob_reduce(pB, nB, k, k, 0, s_g);
    if (threadIdx.x != 0) return;
    const int it = lb->iteration;
    bool all = true, conv[kLobK];
    for (int j = 0; j < k; ++j) {
        const double rn = sqrt(s_r[j * kLobM + j]);
        const double limit = relative ? tol * fabs(lb->theta[j]) : tol;
        conv[j] = rn <= limit;
        all = all && conv[j];
        lb->residual[j] = rn;
        if (trace != nullptr && it < traceCap) trace[(long long)j * traceCap + it] = rn;
    }
    sc->residual = lb->residual[0];
    if (all && it >= minIt) {
        for (int j = 0; j < k; ++j) lb->status[j] = MGCG_OK;
        sc->status = MGCG_OK; sc->done = 1;
        return;
    }
    if (it >= maxIt) {
        for (int j = 0; j < k; ++j) lb->status[j] = conv[j] ? MGCG_OK : MGCG_MAXIT_EXCEEDED;
        sc->status = MGCG_MAXIT_EXCEEDED; sc->done = 1;
        return;
    }
    for (int l = 0; l < k; ++l)
        for (int j = 0; j < k; ++j) lb->CC[l * 2 * kLobK + j] = s_g[l * kLobM + j];
}

// Body, 2: d_a = 1 / sqrt((W^T W)_aa) ; D (W^T W) D = U^T U ; CC = D U^-1 (W = W CC has orthonormal columns)
__global__ __launch_bounds__(kBlock) void lob_w_kernel(LobScalars* lb, CgScalars* sc, const double* __restrict__ pB, int nP, int k)
{
    __shared__ double s_g[kLobM * kLobM], s_u[kLobM * kLobM], s_v[kLobM * kLobM];
    __shared__ double s_d[kLobK];
    if (sc->done != 0) return;
    lob_reduce(pB, nP, k, k, 1, s_g);
    if (threadIdx.x != 0) return;
    for (int a = 0; a < k; ++a) {
        const double g = s_g[a * kLobM + a];
        if (!positive_finite(g)) { lob_fail(lb, sc, k, 2, a); return; }
        s_d[a] = 1.0 / sqrt(g);
    }
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b) { const double t = s_d[a] * s_g[a * kLobM + b]; s_g[a * kLobM + b] = t * s_d[b]; }
    const int bad = lob_cholesky(s_g, s_u, k);
    if (bad >= 0) { lob_fail(lb, sc, k, 2, bad); return; }
    lob_invert_upper(s_u, s_v, k);
    for (int l = 0; l < k; ++l)
        for (int j = 0; j < k; ++j) lb->CC[l * 2 * kLobK + j] = s_d[l] * s_v[l * kLobM + j];
}

// Body, 3: the Rayleigh-Ritz step on S = [X W P] (mHost columns were summed; P takes part when mHost = 3k and no drop is pending)
__global__ __launch_bounds__(kBlock) void lob_basis_kernel(LobScalars* lb, CgScalars* sc, const double* __restrict__ pB, const double* __restrict__ pA, int nP,
                                                           int k, int mHost, int largest)
{
    __shared__ double s_gb[kLobM * kLobM], s_ga[kLobM * kLobM], s_u[kLobM * kLobM], s_ui[kLobM * kLobM], s_t[kLobM * kLobM], s_h[kLobM * kLobM], s_v[kLobM * kLobM];
    __shared__ int s_perm[kLobM];
    if (sc->done != 0) return;
    lob_reduce(pB, nP, mHost, mHost, 1, s_gb);
    lob_reduce(pA, nP, mHost, mHost, 1, s_ga);
    __shared__ int s_m;                                // the order of the problem; 0: the factorisation failed
    if (threadIdx.x == 0) {
        int m = (mHost == 3 * k && lb->skip == 0) ? 3 * k : 2 * k;
        int bad = lob_cholesky(s_gb, s_u, m, m == 3 * k ? kLobDropP : 0.0);
        if (bad >= 0 && m == 3 * k) {                  // drop P for this body and the next
            lb->restarts = lb->restarts + 1; lb->skip = 2;
            m = 2 * k;
            bad = lob_cholesky(s_gb, s_u, m);
        }
        if (bad >= 0) { lob_fail(lb, sc, k, 3, bad); m = 0; }
        else { lob_mirror(s_gb, m); lob_mirror(s_ga, m); lob_invert_upper(s_u, s_ui, m); }
        s_m = m;
    }
    __syncthreads();
    const int m = s_m;
    if (m == 0) return;
    lob_mm<false>(s_ga, s_ui, s_t, m, m, m);           // G_A U^-1
    lob_mm<true>(s_ui, s_t, s_h, m, m, m);             // U^-T (G_A U^-1); its upper triangle is H
    if (threadIdx.x == 0) lob_mirror(s_h, m);
    __syncthreads();
    lob_jacobi(s_h, s_v, m);
    if (threadIdx.x == 0) {
        lob_sort(s_h, m, largest, s_perm);
        for (int l = 0; l < m; ++l)
            for (int j = 0; j < k; ++j) s_t[l * kLobM + j] = s_v[l * kLobM + s_perm[j]];      // Z[:, lowest k]
    }
    __syncthreads();
    double* zs = s_t;
    double* c = s_ga;                                  // C = U^-1 Z[:, lowest k]   (G_A is no longer needed)
    lob_mm<false>(s_ui, zs, c, m, m, k);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < k; ++j) {
        const double w = s_h[s_perm[j] * kLobM + s_perm[j]];
        if (!finite_value(w)) { lob_fail(lb, sc, k, 4, j); return; }
    }
    // Pnew = [W P] C[k:, :] has the squared column norms c_j^T G_B[k:, k:] c_j: its scaling goes into the coefficients
    const int mp = m - k;
    double* gv = s_u;                                  // G_B[k:, k:] C[k:, :]
    for (int a = 0; a < mp; ++a)
        for (int j = 0; j < k; ++j) {
            double s = s_gb[(k + a) * kLobM + k] * c[k * kLobM + j];
            for (int l = 1; l < mp; ++l) { const double t = s_gb[(k + a) * kLobM + k + l] * c[(k + l) * kLobM + j]; s = s + t; }
            gv[a * kLobM + j] = s;
        }
    for (int j = 0; j < k; ++j) {
        double nn = c[k * kLobM + j] * gv[j];
        for (int a = 1; a < mp; ++a) { const double t = c[(k + a) * kLobM + j] * gv[a * kLobM + j]; nn = nn + t; }
        const double scale = positive_finite(nn) ? 1.0 / sqrt(nn) : 0.0;
        for (int l = 0; l < m; ++l) {
            lb->CC[l * 2 * kLobK + j] = c[l * kLobM + j];
            lb->CC[l * 2 * kLobK + k + j] = l >= k ? c[l * kLobM + j] * scale : 0.0;
        }
        lb->theta[j] = s_h[s_perm[j] * kLobM + s_perm[j]];
    }
    lb->mUse = m;
    if (lb->skip > 0) lb->skip = lb->skip - 1;
    lb->iteration = lb->iteration + 1;
}

// Close: trueResidual_j = sqrt(R_j . R_j)
__global__ __launch_bounds__(kBlock) void lob_close_kernel(LobScalars* lb, const double* __restrict__ pR, int nR, int k)
{
    __shared__ double s_r[kLobM * kLobM];
    lob_reduce(pR, nR, k, k, 2, s_r);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < k; ++j) lb->trueResidual[j] = sqrt(s_r[j * kLobM + j]);
}

// ------------------------------------------------------------------ the passes
// X (column stride n) into a block of column stride ld
template <int K>
__global__ __launch_bounds__(kBlock) void lob_copy_kernel(const int* done, double* __restrict__ dst, const double* __restrict__ src, long long n, long long ld)
{
    if (*done != 0) return;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < K; ++j) dst[j * ld + i] = src[j * n + i];
    }
}

// R_j = AX_j - X_j theta_j ; partial sums of R_j . R_j -> entry (j, j) ; PRE 0: W = R, 1: W = dinv o R, 2: W is somebody else's
template <int K, int PRE>
__global__ __launch_bounds__(kBlock) void lob_residual_kernel(const int* done, const LobScalars* __restrict__ lb, const double* __restrict__ X, long long n,
                                                              const double* __restrict__ AX, double* __restrict__ Rv, double* __restrict__ W, long long ld,
                                                              const double* __restrict__ dinv, double* __restrict__ partials)
{
    __shared__ double s_sum[K][4];
    if (*done != 0) return;
    double th[K], h[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { th[j] = lb->theta[j]; h[j] = 0.0; }
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double d = 0.0;
        if constexpr (PRE == 1) d = dinv[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double t = X[j * n + i] * th[j];
            const double r = AX[j * ld + i] - t;
            Rv[j * ld + i] = r;
            if constexpr (PRE == 0) W[j * ld + i] = r;
            if constexpr (PRE == 1) W[j * ld + i] = d * r;
            const double rr = r * r;
            h[j] += rr;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = wave_sum_b(h[j]);
        if ((threadIdx.x & 63) == 0) s_sum[j][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        partials[(long long)(j * kLobM + j) * kLobP + blockIdx.x] = (s_sum[j][0] + s_sum[j][1]) + (s_sum[j][2] + s_sum[j][3]);
    }
}

// Tile (ta, tb) of L^T R: K x K entries, K = the width of a column group
template <int K>
__global__ __launch_bounds__(kBlock) void lob_gram_kernel(const int* done, LobCols L, LobCols Rr, int mR, int upper, long long n, double* __restrict__ partials)
{
    __shared__ double s_sum[K * K][4];
    if (*done != 0) return;
    const int tR = mR / K;
    const int ta = (int)blockIdx.y / tR, tb = (int)blockIdx.y % tR;
    if (upper && ta > tb) return;
    const double* lp[K]; const double* rp[K];
#pragma unroll
    for (int a = 0; a < K; ++a) { lp[a] = L.c[ta * K + a]; rp[a] = Rr.c[tb * K + a]; }
    double h[K * K];
#pragma unroll
    for (int e = 0; e < K * K; ++e) h[e] = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double l[K], r[K];
#pragma unroll
        for (int a = 0; a < K; ++a) { l[a] = lp[a][i]; r[a] = rp[a][i]; }
#pragma unroll
        for (int a = 0; a < K; ++a) {
#pragma unroll
            for (int b = 0; b < K; ++b) { const double t = l[a] * r[b]; h[a * K + b] += t; }
        }
    }
#pragma unroll
    for (int e = 0; e < K * K; ++e) {
        const double t = wave_sum_b(h[e]);
        if ((threadIdx.x & 63) == 0) s_sum[e][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < K * K) {
        const int e = threadIdx.x, a = ta * K + e / K, b = tb * K + e % K;
        partials[(long long)(a * kLobM + b) * kLobP + blockIdx.x] = (s_sum[e][0] + s_sum[e][1]) + (s_sum[e][2] + s_sum[e][3]);
    }
}

// Validation mode (knob dot_order): workgroup a * mR + b forms entry (a, b) as one serial left-to-right sum over the rows of the rounded
// products (bk_gram_serial_kernel's scheme: waves 1-3 stage the products of the next batch in LDS, lane 0 of wave 0 adds the current one).
// mode as lob_reduce's: the entries it skips are not formed.
constexpr int kLobSerialBatch = 2048;
__global__ __launch_bounds__(kBlock) void lob_gram_serial_kernel(const int* done, LobCols L, LobCols Rr, int mR, int mode, long long n, double* __restrict__ partials)
{
    __shared__ double s_prod[2][kLobSerialBatch];
    if (*done != 0) return;
    const int a = (int)blockIdx.x / mR, b = (int)blockIdx.x % mR;
    if ((mode == 1 && a > b) || (mode == 2 && a != b)) return;
    const double* xc = L.c[a];
    const double* yc = Rr.c[b];
    const int tid = threadIdx.x;
    const long long nBatches = (n + kLobSerialBatch - 1) / kLobSerialBatch;
    auto fill = [&](int buf, long long bt) {
        const long long base = bt * kLobSerialBatch;
        for (int q = tid - kWave; q < kLobSerialBatch; q += kBlock - kWave) {
            const long long i = base + q;
            double t = 0.0;
            if (i < n) t = xc[i] * yc[i];
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
            for (int i = 0; i < kLobSerialBatch; ++i) acc += q[i];
        }
        __syncthreads();
    }
    if (tid == 0) partials[(long long)(a * kLobM + b) * kLobP] = acc;
}

// The combine pass.  Family blockIdx.y: out_c[i] = sum over l = l0_c .. mUse-1 of in_l[i] * CC[l][c] for c < MO, with l0_c = 0 for c < pFrom
// and pStart from there on; SUB: out_c[i] = out_c[i] - that sum.  mUse = min(MI, lb->mUse) where the device decides (fromDevice), else MI.
struct LobCombine { LobCols in[2]; LobOut out[2]; int pFrom, pStart, fromDevice; };
template <int MI, int MO, bool SUB>
__global__ __launch_bounds__(kBlock) void lob_combine_kernel(const int* done, const LobScalars* __restrict__ lb, LobCombine job, long long n)
{
    __shared__ double s_c[MI * MO];
    if (*done != 0) return;
    for (int e = threadIdx.x; e < MI * MO; e += kBlock) s_c[e] = lb->CC[(e / MO) * 2 * kLobK + e % MO];
    int mUse = MI;
    if (job.fromDevice) { const int d = lb->mUse; mUse = d < MI ? d : MI; }
    __syncthreads();
    const LobCols& in = job.in[blockIdx.y];
    const LobOut& out = job.out[blockIdx.y];
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double v[MI];                                  // the whole row is in registers before a column of it is overwritten
#pragma unroll
        for (int l = 0; l < MI; ++l) v[l] = l < mUse ? in.c[l][i] : 0.0;
        // one output column per trip, its coefficients read from LDS as it goes: unrolled over c as well, the MI * MO coefficients are hoisted
        // out of the row loop into registers and the wide forms (k >= 6) spill (228 .. 1156 bytes a lane); this form takes 54 VGPRs at k = 8
#pragma unroll 1
        for (int c = 0; c < MO; ++c) {
            const int l0 = c < job.pFrom ? 0 : job.pStart;
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < MI; ++l) {
                if (l < l0 || l >= mUse) continue;
                const double t = v[l] * s_c[l * MO + c];
                s = l == l0 ? t : s + t;
            }
            if constexpr (SUB) out.c[c][i] = out.c[c][i] - s;
            else out.c[c][i] = s;
        }
    }
}

// ------------------------------------------------------------------ launches
static double* lob_pB(Workspace* ws) { return ws->lobPartials; }
static double* lob_pA(Workspace* ws) { return ws->lobPartials + kLobRegion; }
static double* lob_pR(Workspace* ws) { return ws->lobPartials + 2 * (size_t)kLobRegion; }

static int lob_grid(long long n)
{
    const int g = grid_for(n, 1);
    return g < kLobP ? g : kLobP;
}
static LobCols lob_cols(const double* base, long long ld, int k, LobCols c = LobCols{}, int at = 0)
{
    for (int j = 0; j < k; ++j) c.c[at + j] = base + j * ld;
    return c;
}
static LobOut lob_outs(double* base, long long ld, int k, LobOut c = LobOut{}, int at = 0)
{
    for (int j = 0; j < k; ++j) c.c[at + j] = base + j * ld;
    return c;
}

// L^T R into `partials`; mode as lob_reduce's; returns the partial sums per entry (1 under dot_order = 1)
template <int K>
static int lob_gram(hipStream_t s, const int* done, const LobCols& L, const LobCols& Rr, int mL, int mR, int mode, long long n, double* partials)
{
    if (dot_reference_order()) {
        hipLaunchKernelGGL(lob_gram_serial_kernel, dim3(mL * mR), dim3(kBlock), 0, s, done, L, Rr, mR, mode, n, partials);
        return 1;
    }
    const int g = lob_grid(n);
    hipLaunchKernelGGL((lob_gram_kernel<K>), dim3(g, (mL / K) * (mR / K)), dim3(kBlock), 0, s, done, L, Rr, mR, mode == 1 ? 1 : 0, n, partials);
    return g;
}

template <int MI, int MO, bool SUB>
static void lob_combine(hipStream_t s, const int* done, const LobScalars* lb, const LobCombine& job, int families, long long n)
{
    hipLaunchKernelGGL((lob_combine_kernel<MI, MO, SUB>), dim3(grid_for(n, 1), families), dim3(kBlock), 0, s, done, lb, job, n);
}

// X = X CC, AX = AX CC in place (CC k x k)
template <int K>
static void lob_transform_x(const LobRun& R, const int* done)
{
    LobCombine job{};
    job.in[0] = lob_cols(R.X, R.n, K); job.out[0] = lob_outs(R.X, R.n, K);
    job.in[1] = lob_cols(R.AX, R.ld, K); job.out[1] = lob_outs(R.AX, R.ld, K);
    job.pFrom = K; job.pStart = 0; job.fromDevice = 0;
    lob_combine<K, K, false>(R.ws->stream, done, R.ws->lobScalars, job, 2, R.n);
}

// the residual pass; returns the partial sums per column in lob_pR (entry (j, j))
template <int K>
static int lob_residual(const LobRun& R, const int* done, int pre)
{
    hipStream_t s = R.ws->stream;
    const int g = lob_grid(R.n);
    const LobScalars* lb = R.ws->lobScalars;
#define GO(PRE) hipLaunchKernelGGL((lob_residual_kernel<K, PRE>), dim3(g), dim3(kBlock), 0, s, done, lb, (const double*)R.X, R.n, (const double*)R.AX, R.Rv, R.W, R.ld, R.dinv, lob_pR(R.ws))
    if (pre == 0) GO(0); else if (pre == 1) GO(1); else GO(2);
#undef GO
    if (!dot_reference_order()) return g;
    const LobCols rc = lob_cols(R.Rv, R.ld, K);
    return lob_gram<K>(s, done, rc, rc, K, K, 2, R.n, lob_pR(R.ws));
}

template <int K>
static bool lob_enqueue_start_k(const LobRun& R)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const int* done = &ws->scalars->done;
    // AX = A X through P's block (P is absent until the first body ends): the product's operands lie ld apart
    hipLaunchKernelGGL((lob_copy_kernel<K>), dim3(grid_for(R.n, 1)), dim3(kBlock), 0, s, done, R.P, (const double*)R.X, R.n, R.ld);
    launch_spmv_block_plain(s, K, R.elements, R.rowOffsets, R.columnIndeces, R.P, R.AX, R.ld, R.n, done);
    const LobCols xc = lob_cols(R.X, R.n, K), axc = lob_cols(R.AX, R.ld, K);
    int nP = lob_gram<K>(s, done, xc, xc, K, K, 1, R.n, lob_pB(ws));
    hipLaunchKernelGGL(lob_start_kernel, dim3(1), dim3(kBlock), 0, s, ws->lobScalars, ws->scalars, (const double*)lob_pB(ws), nP, K);
    lob_transform_x<K>(R, done);
    nP = lob_gram<K>(s, done, xc, axc, K, K, 1, R.n, lob_pA(ws));
    hipLaunchKernelGGL(lob_ritz0_kernel, dim3(1), dim3(kBlock), 0, s, ws->lobScalars, ws->scalars, (const double*)lob_pA(ws), nP, K, R.largest);
    lob_transform_x<K>(R, done);
    return MGCG_HIP(hipGetLastError());
}

template <int K>
static bool lob_enqueue_rest_k(const LobRun& R, int body, int nR)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    CgScalars* sc = ws->scalars;
    const int* done = &sc->done;
    LobScalars* lb = ws->lobScalars;
    const LobCols xc = lob_cols(R.X, R.n, K), wc = lob_cols(R.W, R.ld, K);
    // X^T W, the judgement ; W = W - X (X^T W)
    int nB = lob_gram<K>(s, done, xc, wc, K, K, 0, R.n, lob_pB(ws));
    hipLaunchKernelGGL(lob_judge_kernel, dim3(1), dim3(kBlock), 0, s, lb, sc, (const double*)lob_pR(ws), nR, (const double*)lob_pB(ws), nB, K, R.tol, R.relative, R.minIt, R.maxIt,
                       R.trace, R.traceCap);
    {
        LobCombine job{};
        job.in[0] = xc; job.out[0] = lob_outs(R.W, R.ld, K);
        job.pFrom = K; job.pStart = 0; job.fromDevice = 0;
        lob_combine<K, K, true>(s, done, lb, job, 1, R.n);
    }
    // W^T W = (D^-1 U^T)(U D^-1) ; W = W D U^-1
    nB = lob_gram<K>(s, done, wc, wc, K, K, 1, R.n, lob_pB(ws));
    hipLaunchKernelGGL(lob_w_kernel, dim3(1), dim3(kBlock), 0, s, lb, sc, (const double*)lob_pB(ws), nB, K);
    {
        LobCombine job{};
        job.in[0] = wc; job.out[0] = lob_outs(R.W, R.ld, K);
        job.pFrom = K; job.pStart = 0; job.fromDevice = 0;
        lob_combine<K, K, false>(s, done, lb, job, 1, R.n);
    }
    launch_spmv_block_plain(s, K, R.elements, R.rowOffsets, R.columnIndeces, R.W, R.AW, R.ld, R.n, done);     // AW = A W
    // G_B = S^T S, G_A = S^T AS over S = [X W P] (body 0: [X W]) ; the dense step ; X, AX, P, AP
    const int m = body == 0 ? 2 * K : 3 * K;
    LobCols sc3 = lob_cols(R.W, R.ld, K, xc, K), as3 = lob_cols(R.AW, R.ld, K, lob_cols(R.AX, R.ld, K), K);
    sc3 = lob_cols(R.P, R.ld, K, sc3, 2 * K); as3 = lob_cols(R.AP, R.ld, K, as3, 2 * K);
    nB = lob_gram<K>(s, done, sc3, sc3, m, m, 1, R.n, lob_pB(ws));
    (void)lob_gram<K>(s, done, sc3, as3, m, m, 1, R.n, lob_pA(ws));
    hipLaunchKernelGGL(lob_basis_kernel, dim3(1), dim3(kBlock), 0, s, lb, sc, (const double*)lob_pB(ws), (const double*)lob_pA(ws), nB, K, m, R.largest);
    {
        LobCombine job{};
        job.in[0] = sc3; job.in[1] = as3;
        job.out[0] = lob_outs(R.P, R.ld, K, lob_outs(R.X, R.n, K), K);
        job.out[1] = lob_outs(R.AP, R.ld, K, lob_outs(R.AX, R.ld, K), K);
        job.pFrom = K; job.pStart = K; job.fromDevice = 1;
        lob_combine<3 * K, 2 * K, false>(s, done, lb, job, 2, R.n);
    }
    return MGCG_HIP(hipGetLastError());
}

template <int K>
static bool lob_enqueue_close_k(const LobRun& R)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const int* never = &ws->lobScalars->zero;
    hipLaunchKernelGGL((lob_copy_kernel<K>), dim3(grid_for(R.n, 1)), dim3(kBlock), 0, s, never, R.W, (const double*)R.X, R.n, R.ld);
    launch_spmv_block_plain(s, K, R.elements, R.rowOffsets, R.columnIndeces, R.W, R.AX, R.ld, R.n, nullptr);
    const int nR = lob_residual<K>(R, never, 2);
    hipLaunchKernelGGL(lob_close_kernel, dim3(1), dim3(kBlock), 0, s, ws->lobScalars, (const double*)lob_pR(ws), nR, K);
    return MGCG_HIP(hipGetLastError());
}

bool lob_enqueue_start(const LobRun& R) { return dispatch_k(R.k, [&](auto K) { return lob_enqueue_start_k<K.value>(R); }); }
int lob_enqueue_residual(const LobRun& R) { return dispatch_k(R.k, [&](auto K) { return lob_residual<K.value>(R, &R.ws->scalars->done, R.pre); }); }
bool lob_enqueue_rest(const LobRun& R, int body, int nR) { return dispatch_k(R.k, [&](auto K) { return lob_enqueue_rest_k<K.value>(R, body, nR); }); }
bool lob_enqueue_close(const LobRun& R) { return dispatch_k(R.k, [&](auto K) { return lob_enqueue_close_k<K.value>(R); }); }

bool lob_read_results(Workspace* ws, int k, LobResult* out)
{
    LobScalars h;
    if (!MGCG_HIP(hipMemcpy(&h, ws->lobScalars, sizeof(h), hipMemcpyDeviceToHost))) return false;
    out->iteration = h.iteration; out->restarts = h.restarts; out->failWhich = h.failWhich; out->failPivot = h.failPivot;
    for (int j = 0; j < k; ++j) { out->theta[j] = h.theta[j]; out->residual[j] = h.residual[j]; out->trueResidual[j] = h.trueResidual[j]; out->status[j] = h.status[j]; }
    return true;
}

void preload_kernels_lobpcg() { preload_code_object(reinterpret_cast<const void*>(&lob_start_kernel)); }

} // namespace mgcg
