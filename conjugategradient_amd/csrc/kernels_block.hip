// Block CG for gfx950: k = 1..8 independent CG recurrences on ONE matrix, every iteration reading the matrix once for all k
// (SolveBlockEx), and the block product y = A x for k columns (CsrMVBlock).  Plain CSR only, one rank, no preconditioner.
//
// Layout.  x, b, r (and CsrMVBlock's x, y) are the caller's: column j at [j*count, (j+1)*count).  The loop's own p and Ap are
// row-interleaved, p[i*k + j]: one gathered column id then fetches the k doubles of that row with 16-byte loads (k even) instead of
// k separate gathers, and the own-row operand of the p.Ap epilogue is one contiguous load as well.
//
// Arithmetic.  Every row adds its products in stored order, each product rounded before it is added (-ffp-contract=off), starting
// from +0.0: column j of a block product is bit-identical to the stored-order product of column j alone (oracle.spmv, the lane = row
// CSR kernels).  The vector passes use the single-vector loop's rounded operations (kernels_blas1.hip): r = r + (-alpha) Ap,
// x = x + alpha p, p = r + beta p.  Dot products are per-column tree sums of per-workgroup partials; with dot_order = 1 every one of
// them is a serial left-to-right sum (block_dot_serial_kernel), which is the oracle's arithmetic, so every column then EQUALS the
// oracle's CG on that column alone.  The stop decision is decide_stop (common.hpp), per column.
//
// Frozen columns.  The finalisation kernel gives every column a mode for the x/p pass of its iteration: 2 = x and p (the column goes
// on), 1 = x only (the column stopped in this iteration), 0 = nothing (it had stopped before).  A column that stopped is inactive from
// then on: no kernel writes its x, r or p again and its trace gets no entry.  Its Ap is still formed by the block product (the matrix
// is read anyway; Ap is work space).  The device stop flag rises when no column is active.
#include "common.hpp"

namespace mgcg {

typedef double d2 __attribute__((ext_vector_type(2)));

struct BlockScalars {
    double rr[kBlockMaxK], rr0[kBlockMaxK], alpha[kBlockMaxK], beta[kBlockMaxK], residual[kBlockMaxK];
    int iteration[kBlockMaxK], status[kBlockMaxK], active[kBlockMaxK], mode[kBlockMaxK];
    int done, pad;
};

bool Workspace::ensure_block()
{
    if (blockPartials && blockScalars) return true;
    if (!blockPartials && !MGCG_HIP(hipMalloc((void**)&blockPartials, sizeof(double) * 3 * kBlockMaxK * (size_t)kMaxPartials))) return false;
    if (!blockScalars) {
        if (!MGCG_HIP(hipMalloc((void**)&blockScalars, sizeof(BlockScalars)))) return false;
        if (!MGCG_HIP(hipMemset(blockScalars, 0, sizeof(BlockScalars)))) return false;
    }
    return true;
}

// ------------------------------------------------------------------ row loads of the interleaved vectors
template <int K, bool NT = false>
__device__ __forceinline__ void load_row(const double* p, double (&v)[K])
{
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int j = 0; j < K / 2; ++j) {
            d2 t;
            if constexpr (NT) t = __builtin_nontemporal_load((const d2*)p + j); else t = ((const d2*)p)[j];
            v[2 * j] = t.x; v[2 * j + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) { if constexpr (NT) v[j] = __builtin_nontemporal_load(p + j); else v[j] = p[j]; }
    }
}
template <int K, bool NT = false>
__device__ __forceinline__ void store_row(double* p, const double (&v)[K])
{
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int j = 0; j < K / 2; ++j) {
            d2 t; t.x = v[2 * j]; t.y = v[2 * j + 1];
            if constexpr (NT) __builtin_nontemporal_store(t, (d2*)p + j); else ((d2*)p)[j] = t;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) { if constexpr (NT) __builtin_nontemporal_store(v[j], p + j); else p[j] = v[j]; }
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { double o = __shfl_down(v, off, 64); v = o > v ? o : v; }
    return v;
}
// Fixed-order sum (mode 0) or max (mode 1) of n partials by one workgroup; result valid in every thread.
__device__ double block_reduce(const double* __restrict__ partials, int n, double* s_red, int mode)
{
    double acc = 0.0;
    if (mode == 0) { for (int i = threadIdx.x; i < n; i += kBlock) acc += partials[i]; acc = wave_sum(acc); }
    else { for (int i = threadIdx.x; i < n; i += kBlock) { double a = partials[i]; acc = a > acc ? a : acc; } acc = wave_max(acc); }
    __syncthreads();                                        // (s_red is reused by consecutive calls)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (mode == 0) return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    double a = s_red[0] > s_red[1] ? s_red[0] : s_red[1];
    double b = s_red[2] > s_red[3] ? s_red[2] : s_red[3];
    return a > b ? a : b;
}

// ------------------------------------------------------------------ block SpMV
// A workgroup of four wavefronts takes one tile of 256 consecutive rows per trip, lane = row.  Every wavefront stages the raw
// column ids and values of its 64 rows (one contiguous span of the CSR arrays) in LDS with coalesced loads -- non-temporal in the
// CG loop, as the row-tile kernel's flag 8 -- and, when no row of the 64 is longer than kBNG, issues all gathers of a row at once
// (masked slots read column 0 and add +0.0, which changes no bit: a sum that starts at +0.0 is never -0.0).  Longer rows and spans
// that do not fit take a loop over the entries.
constexpr int kBTW = 4;
constexpr int kBTRows = 64 * kBTW;
constexpr int kBTCap = 512;
constexpr int kBNG = 8;

enum { BEPI_AP = 0,          // x interleaved; y interleaved = A x; partial[j] += x_j[row] * y_j[row]   (Ap = A p ; p.Ap)
       BEPI_RESIDUAL = 1,    // x, y, b column-major; y_j = b_j - A x_j
       BEPI_PLAIN = 2,       // x, y column-major; y_j = A x_j
       BEPI_GRAM = 3 };      // x interleaved; y interleaved = A x; partial[(a, b)] += x_a[row] * y_b[row], a <= b   (T = A S ; S^T T, kernels_bkrylov.hip)

struct BlockSpmvArgs {
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    const double* x;
    double* y;
    const double* b;
    long long ld;            // column stride of the column-major operands
    int rows;
    double* partials;        // BEPI_AP: column j's partial sums at partials + j * kMaxPartials, one per wavefront
                             // BEPI_GRAM: the same per entry (a, b), a <= b, of the upper triangle in row-major order (gram_index)
    const int* done;
};

template <int K, int EPI>
__device__ __forceinline__ void gather(const BlockSpmvArgs& a, int col, double (&v)[K])
{
    if constexpr (EPI == BEPI_AP || EPI == BEPI_GRAM) load_row<K>(a.x + (long long)col * K, v);
    else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = a.x[j * a.ld + col];
    }
}

template <int K, int EPI, bool NT>
__global__ __launch_bounds__(64 * kBTW) void spmv_block_kernel(BlockSpmvArgs a)
{
    __shared__ __attribute__((aligned(16))) int s_colAll[kBTCap * kBTW];
    __shared__ __attribute__((aligned(16))) double s_valAll[kBTCap * kBTW];
    if (a.done != nullptr && *a.done != 0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int* s_col = s_colAll + wv * kBTCap;
    double* s_val = s_valAll + wv * kBTCap;
    const int nTiles = (a.rows + kBTRows - 1) / kBTRows;
    constexpr int nDot = EPI == BEPI_GRAM ? K * (K + 1) / 2 : K;
    double dot[nDot];
#pragma unroll
    for (int j = 0; j < nDot; ++j) dot[j] = 0.0;
    for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {       // workgroup-uniform trip count: the barriers below are safe
        const int r0 = tile * kBTRows + wv * 64;
        const int row = r0 + lane;
        const bool valid = row < a.rows;
        const int rb = r0 < a.rows ? r0 : a.rows;
        const int rl = r0 + 64 < a.rows ? r0 + 64 : a.rows;
        const int s = a.rowOffsets[rb];
        const int e = a.rowOffsets[rl > rb ? rl : rb];
        const int rs = valid ? a.rowOffsets[row] : 0;
        const int re = valid ? a.rowOffsets[row + 1] : 0;
        const int cnt = re - rs;
        const bool staged = e - s <= kBTCap;                               // wavefront-uniform
        if (staged) {
            for (int q = lane; q < e - s; q += 64) {
                if constexpr (NT) { s_col[q] = __builtin_nontemporal_load(a.columnIndeces + s + q); s_val[q] = __builtin_nontemporal_load(a.elements + s + q); }
                else { s_col[q] = a.columnIndeces[s + q]; s_val[q] = a.elements[s + q]; }
            }
        }
        __syncthreads();
        const bool fast = staged && __ballot(cnt > kBNG) == 0ull;
        double acc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = 0.0;
        if (fast) {
            int cc[kBNG]; double vv[kBNG];
#pragma unroll
            for (int q = 0; q < kBNG; ++q) {
                const bool in = q < cnt;
                const int idx = in ? rs - s + q : 0;
                const int c = s_col[idx]; const double v = s_val[idx];
                cc[q] = in ? c : 0; vv[q] = in ? v : 0.0;
            }
            double xg[kBNG][K];
#pragma unroll
            for (int q = 0; q < kBNG; ++q) gather<K, EPI>(a, cc[q], xg[q]);
#pragma unroll
            for (int q = 0; q < kBNG; ++q) {
#pragma unroll
                for (int j = 0; j < K; ++j) { const double t = vv[q] * xg[q][j]; acc[j] += (q < cnt) ? t : 0.0; }
            }
        } else if (valid) {
            for (int q = rs; q < re; ++q) {
                int col; double v;
                if (staged) { col = s_col[q - s]; v = s_val[q - s]; }
                else if constexpr (NT) { col = __builtin_nontemporal_load(a.columnIndeces + q); v = __builtin_nontemporal_load(a.elements + q); }
                else { col = a.columnIndeces[q]; v = a.elements[q]; }
                double xv[K];
                gather<K, EPI>(a, col, xv);
#pragma unroll
                for (int j = 0; j < K; ++j) { const double t = v * xv[j]; acc[j] += t; }
            }
        }
        if (valid) {
            if constexpr (EPI == BEPI_AP) {
                double w[K];
                load_row<K>(a.x + (long long)row * K, w);
#pragma unroll
                for (int j = 0; j < K; ++j) { const double t = w[j] * acc[j]; dot[j] += t; }
                store_row<K, NT>(a.y + (long long)row * K, acc);
            } else if constexpr (EPI == BEPI_GRAM) {
                double w[K];
                load_row<K>(a.x + (long long)row * K, w);
                int e = 0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
#pragma unroll
                    for (int j = i; j < K; ++j) { const double t = w[i] * acc[j]; dot[e] += t; ++e; }
                }
                store_row<K, NT>(a.y + (long long)row * K, acc);
            } else if constexpr (EPI == BEPI_RESIDUAL) {
#pragma unroll
                for (int j = 0; j < K; ++j) a.y[j * a.ld + row] = a.b[j * a.ld + row] - acc[j];
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) a.y[j * a.ld + row] = acc[j];
            }
        }
        __syncthreads();                                                   // the next trip overwrites the staged span
    }
    if constexpr (EPI == BEPI_AP || EPI == BEPI_GRAM) {
#pragma unroll
        for (int j = 0; j < nDot; ++j) {
            const double t = wave_sum(dot[j]);
            if (lane == 0) a.partials[(long long)j * kMaxPartials + blockIdx.x * kBTW + wv] = t;
        }
    }
}

// returns the number of partial sums per column (BEPI_AP)
template <int K>
static int launch_spmv_block(hipStream_t s, int epi, const BlockSpmvArgs& a, bool nt)
{
    if (a.rows <= 0) return 0;
    const int nTiles = (a.rows + kBTRows - 1) / kBTRows;
    DeviceState* d = device_state();
    int nWG = 2 * (d ? d->numCu : kNumCu);                                 // 8 wavefronts per CU, as the row-tile kernel
    if (nWG > nTiles) nWG = nTiles;
    if (nWG * kBTW > kMaxPartials) nWG = kMaxPartials / kBTW;
#define GO(E, N) hipLaunchKernelGGL((spmv_block_kernel<K, E, N>), dim3(nWG), dim3(64 * kBTW), 0, s, a)
    if (epi == BEPI_AP) { if (nt) GO(BEPI_AP, true); else GO(BEPI_AP, false); }
    else if (epi == BEPI_RESIDUAL) { if (nt) GO(BEPI_RESIDUAL, true); else GO(BEPI_RESIDUAL, false); }
    else { if (nt) GO(BEPI_PLAIN, true); else GO(BEPI_PLAIN, false); }
#undef GO
    return nWG * kBTW;
}

// T = A S with the partial sums of the upper triangle of S^T T (shared-subspace block CG, kernels_bkrylov.hip); returns their count per entry
template <int K>
static int spmv_block_gram(hipStream_t s, const BlockSpmvArgs& a, bool nt)
{
    const int nTiles = (a.rows + kBTRows - 1) / kBTRows;
    DeviceState* d = device_state();
    int nWG = 2 * (d ? d->numCu : kNumCu);
    if (nWG > nTiles) nWG = nTiles;
    if (nWG * kBTW > kMaxPartials) nWG = kMaxPartials / kBTW;
    if (nt) hipLaunchKernelGGL((spmv_block_kernel<K, BEPI_GRAM, true>), dim3(nWG), dim3(64 * kBTW), 0, s, a);
    else hipLaunchKernelGGL((spmv_block_kernel<K, BEPI_GRAM, false>), dim3(nWG), dim3(64 * kBTW), 0, s, a);
    return nWG * kBTW;
}

int launch_spmv_block_gram(hipStream_t s, int k, const double* elements, const int* rowOffsets, const int* columnIndeces,
                           const double* S, double* T, long long rows, double* gramPartials, const int* done)
{
    if (rows <= 0) return 0;
    BlockSpmvArgs a{};
    a.elements = elements; a.rowOffsets = rowOffsets; a.columnIndeces = columnIndeces;
    a.x = S; a.y = T; a.ld = rows; a.rows = (int)rows; a.partials = gramPartials; a.done = done;
    const bool nt = rows >= 8000000;                   // (the block loop's rule: block_nt)
    return dispatch_k(k, [&](auto K) { return spmv_block_gram<K.value>(s, a, nt); });
}

// ------------------------------------------------------------------ vector passes
static int vec_grid(long long n)
{
    long long g = (n + kBlock - 1) / kBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// per-column block sums of acc[K] (and mx[K]) -> partials[j * kMaxPartials + blockIdx.x]
template <int K, bool INF>
__device__ __forceinline__ void block_partials_out(double (&acc)[K], double (&mx)[K], double* partials, double* partialsInf)
{
    __shared__ double s_sum[K][4];
    __shared__ double s_max[K][4];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double t = wave_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) s_sum[j][threadIdx.x >> 6] = t;
        if constexpr (INF) { const double m = wave_max(mx[j]); if ((threadIdx.x & 63) == 0) s_max[j][threadIdx.x >> 6] = m; }
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        partials[(long long)j * kMaxPartials + blockIdx.x] = (s_sum[j][0] + s_sum[j][1]) + (s_sum[j][2] + s_sum[j][3]);
        if constexpr (INF) {
            double a = s_max[j][0] > s_max[j][1] ? s_max[j][0] : s_max[j][1];
            double b = s_max[j][2] > s_max[j][3] ? s_max[j][2] : s_max[j][3];
            partialsInf[(long long)j * kMaxPartials + blockIdx.x] = a > b ? a : b;
        }
    }
}

// init: p = interleave(r) ; partial r_j.r_j
template <int K>
__global__ __launch_bounds__(kBlock) void block_copy_dot_kernel(double* __restrict__ p, const double* __restrict__ r, long long n, double* __restrict__ partials)
{
    double acc[K], mx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { acc[j] = 0.0; mx[j] = 0.0; }
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double pv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { const double rv = r[j * n + i]; pv[j] = rv; const double t = rv * rv; acc[j] += t; }
        store_row<K>(p + i * K, pv);
    }
    block_partials_out<K, false>(acc, mx, partials, nullptr);
}

// r_j = r_j + (-alpha_j) Ap_j ; partial r_j.r_j [, max |r_j|]   (active columns only)
template <int K, bool INF, bool NT>
__global__ __launch_bounds__(kBlock) void block_update_r_kernel(const BlockScalars* __restrict__ sc, double* __restrict__ r, const double* __restrict__ Ap, long long n,
                                                                double* __restrict__ partials, double* __restrict__ partialsInf)
{
    if (sc->done != 0) return;
    bool act[K]; double malpha[K], acc[K], mx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { act[j] = sc->active[j] != 0; malpha[j] = -sc->alpha[j]; acc[j] = 0.0; mx[j] = 0.0; }
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double av[K];
        load_row<K, NT>(Ap + i * K, av);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (!act[j]) continue;
            const double u = malpha[j] * av[j]; const double rv = r[j * n + i] + u; r[j * n + i] = rv;
            const double q = rv * rv; acc[j] += q;
            if constexpr (INF) { const double a0 = fabs(rv); mx[j] = a0 > mx[j] ? a0 : mx[j]; }
        }
    }
    block_partials_out<K, INF>(acc, mx, partials, partialsInf);
}

// x_j = x_j + alpha_j p_j (mode >= 1) ; p_j = r_j + beta_j p_j (mode 2)
template <int K, bool NT>
__global__ __launch_bounds__(kBlock) void block_update_xp_kernel(const BlockScalars* __restrict__ sc, double* __restrict__ x, double* __restrict__ p,
                                                                 const double* __restrict__ r, long long n)
{
    int mode[K]; double al[K], be[K];
    bool any = false, anyP = false;
#pragma unroll
    for (int j = 0; j < K; ++j) { mode[j] = sc->mode[j]; al[j] = sc->alpha[j]; be[j] = sc->beta[j]; any = any || mode[j] > 0; anyP = anyP || mode[j] == 2; }
    if (!any) return;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        double pv[K];
        load_row<K, NT>(p + i * K, pv);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (mode[j] == 0) continue;
            const double t = al[j] * pv[j]; x[j * n + i] = x[j * n + i] + t;
            if (mode[j] == 2) { const double u = be[j] * pv[j]; pv[j] = r[j * n + i] + u; }
        }
        if (anyP) store_row<K, NT>(p + i * K, pv);          // (frozen columns write back the bits they read)
    }
}

// ------------------------------------------------------------------ validation mode: serial dots per column (knob dot_order)
// Column j = blockIdx.x: sum over i of x[j*colStep + i*elemStep] * y[...], rounded products added strictly left to right
// (dot_serial_kernel's scheme: waves 1-3 stage the products of the next batch in LDS, lane 0 of wave 0 adds the current one).
constexpr int kBSerialBatch = 2048;
__global__ __launch_bounds__(kBlock) void block_dot_serial_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                                  long long colStep, long long elemStep, double* __restrict__ out, const BlockScalars* sc)
{
    __shared__ double s_prod[2][kBSerialBatch];
    const int col = blockIdx.x;
    if (sc != nullptr && (sc->done != 0 || sc->active[col] == 0)) return;
    const double* xc = x + col * colStep;
    const double* yc = y + col * colStep;
    const int tid = threadIdx.x;
    const long long nBatches = (n + kBSerialBatch - 1) / kBSerialBatch;
    auto fill = [&](int buf, long long b) {
        const long long base = b * kBSerialBatch;
        for (int k = tid - kWave; k < kBSerialBatch; k += kBlock - kWave) {
            const long long i = base + k;
            double t = 0.0;
            if (i < n) t = xc[i * elemStep] * yc[i * elemStep];
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
            for (int k = 0; k < kBSerialBatch; ++k) acc += q[k];
        }
        __syncthreads();
    }
    if (tid == 0) out[(long long)col * kMaxPartials] = acc;
}

// ------------------------------------------------------------------ scalar kernels (one workgroup)
__global__ __launch_bounds__(kBlock) void block_init_kernel(BlockScalars* sc, const double* __restrict__ partials, int n, int k)
{
    __shared__ double s_red[4];
    for (int j = 0; j < kBlockMaxK; ++j) {
        const double rr = j < k ? block_reduce(partials + (long long)j * kMaxPartials, n, s_red, 0) : 0.0;
        if (threadIdx.x == 0) {
            sc->rr[j] = rr; sc->rr0[j] = rr; sc->alpha[j] = 0.0; sc->beta[j] = 0.0; sc->residual[j] = 0.0;
            sc->iteration[j] = 0; sc->status[j] = MGCG_OK; sc->active[j] = j < k ? 1 : 0; sc->mode[j] = 0;
        }
    }
    if (threadIdx.x == 0) { sc->done = k > 0 ? 0 : 1; sc->pad = 0; }
}

// alpha_j = rr_j / p_j.Ap_j
__global__ __launch_bounds__(kBlock) void block_alpha_kernel(BlockScalars* sc, const double* __restrict__ partials, int n, int k)
{
    __shared__ double s_red[4];
    if (sc->done != 0) return;
    for (int j = 0; j < k; ++j) {
        if (sc->active[j] == 0) continue;                                  // (uniform: every thread reads the same flag)
        const double pAp = block_reduce(partials + (long long)j * kMaxPartials, n, s_red, 0);
        if (threadIdx.x == 0) sc->alpha[j] = sc->rr[j] / pAp;
    }
}

// Per active column: the residual, the stop decision of its iteration, its trace entry, beta and the mode of the x/p pass.
__global__ __launch_bounds__(kBlock) void block_finalize_kernel(BlockScalars* sc, const double* __restrict__ partials, int n,
                                                                const double* __restrict__ partialsInf, int nInf, int k, FinalizeArgs f)
{
    __shared__ double s_red[4];
    if (sc->done != 0) { if (threadIdx.x < kBlockMaxK) sc->mode[threadIdx.x] = 0; return; }
    for (int j = 0; j < k; ++j) {
        if (sc->active[j] == 0) { if (threadIdx.x == 0) sc->mode[j] = 0; continue; }
        const double rrNew = block_reduce(partials + (long long)j * kMaxPartials, n, s_red, 0);
        const double inf = partialsInf != nullptr ? block_reduce(partialsInf + (long long)j * kMaxPartials, nInf, s_red, 1) : 0.0;
        if (threadIdx.x == 0) {
            const int it = sc->iteration[j];
            const StopDecision d = decide_stop(f, rrNew, inf, sc->rr0[j], it);
            if (f.trace != nullptr && it < f.traceCap) f.trace[(long long)j * f.traceCap + it] = d.shown;
            sc->residual[j] = d.res;
            if (d.stop) { sc->mode[j] = 1; sc->active[j] = 0; sc->status[j] = d.status; }
            else { sc->mode[j] = 2; sc->beta[j] = rrNew / sc->rr[j]; sc->rr[j] = rrNew; sc->iteration[j] = it + 1; }
        }
    }
    if (threadIdx.x == 0) {
        int any = 0;
        for (int j = 0; j < k; ++j) any |= sc->active[j];
        sc->done = any ? 0 : 1;
    }
}

__global__ void block_snapshot_kernel(const BlockScalars* sc, volatile int* slot) { *slot = sc->done; }

// ------------------------------------------------------------------ the loop's launches (its host side is cg_solve_block, solver.hip)
static bool block_nt(const BlockRun& R) { return R.n >= 8000000; }   // the streaming hints of the CG loop's passes (vectors and matrix far beyond the caches)

template <int K>
static bool block_enqueue_start_k(const BlockRun& R)
{
    hipStream_t s = R.ws->stream;
    double* P0 = R.ws->blockPartials;
    if (R.rule == MGCG_RULE_SIMPLE) launch_fill(s, R.x, 0.0, K * R.n);                    // SimpleConjugateGradient.cu:53, per column
    BlockSpmvArgs a{};
    a.elements = R.elements; a.rowOffsets = R.rowOffsets; a.columnIndeces = R.columnIndeces;
    a.x = R.x; a.y = R.r; a.b = R.b; a.ld = R.n; a.rows = (int)R.n;
    (void)launch_spmv_block<K>(s, BEPI_RESIDUAL, a, block_nt(R));                          // r_j = b_j - A x_j
    const int g = vec_grid(R.n);
    hipLaunchKernelGGL((block_copy_dot_kernel<K>), dim3(g), dim3(kBlock), 0, s, R.p, R.r, R.n, P0);   // p = r ; r.r
    int nP = g;
    if (dot_reference_order()) {
        hipLaunchKernelGGL(block_dot_serial_kernel, dim3(K), dim3(kBlock), 0, s, R.r, R.r, R.n, R.n, 1LL, P0, (const BlockScalars*)nullptr);
        nP = 1;
    }
    hipLaunchKernelGGL(block_init_kernel, dim3(1), dim3(kBlock), 0, s, R.ws->blockScalars, P0, nP, K);
    return MGCG_HIP(hipGetLastError());
}

template <int K>
static bool block_enqueue_iteration_k(const BlockRun& R, const FinalizeArgs& f)
{
    hipStream_t s = R.ws->stream;
    BlockScalars* sc = R.ws->blockScalars;
    double* P0 = R.ws->blockPartials;
    double* P1 = P0 + (size_t)kBlockMaxK * kMaxPartials;
    double* P2 = P1 + (size_t)kBlockMaxK * kMaxPartials;
    const bool ref = dot_reference_order();
    const bool inf = R.rule == MGCG_RULE_HANDMADECL;
    const bool nt = block_nt(R);
    BlockSpmvArgs a{};
    a.elements = R.elements; a.rowOffsets = R.rowOffsets; a.columnIndeces = R.columnIndeces;
    a.x = R.p; a.y = R.Ap; a.ld = R.n; a.rows = (int)R.n; a.partials = P0; a.done = &sc->done;
    int nPAp = launch_spmv_block<K>(s, BEPI_AP, a, nt);                                      // Ap = A p ; p_j.Ap_j
    if (ref) { hipLaunchKernelGGL(block_dot_serial_kernel, dim3(K), dim3(kBlock), 0, s, R.p, R.Ap, R.n, 1LL, (long long)K, P0, (const BlockScalars*)sc); nPAp = 1; }
    hipLaunchKernelGGL(block_alpha_kernel, dim3(1), dim3(kBlock), 0, s, sc, P0, nPAp, K);   // alpha_j
    const int g = vec_grid(R.n);
#define GO(I, N) hipLaunchKernelGGL((block_update_r_kernel<K, I, N>), dim3(g), dim3(kBlock), 0, s, sc, R.r, R.Ap, R.n, P1, P2)
    if (inf) { if (nt) GO(true, true); else GO(true, false); }
    else { if (nt) GO(false, true); else GO(false, false); }
#undef GO
    int nRR = g;
    if (ref) { hipLaunchKernelGGL(block_dot_serial_kernel, dim3(K), dim3(kBlock), 0, s, R.r, R.r, R.n, R.n, 1LL, P1, (const BlockScalars*)sc); nRR = 1; }
    hipLaunchKernelGGL(block_finalize_kernel, dim3(1), dim3(kBlock), 0, s, sc, P1, nRR, inf ? P2 : nullptr, g, K, f);
    if (nt) hipLaunchKernelGGL((block_update_xp_kernel<K, true>), dim3(g), dim3(kBlock), 0, s, sc, R.x, R.p, R.r, R.n);
    else hipLaunchKernelGGL((block_update_xp_kernel<K, false>), dim3(g), dim3(kBlock), 0, s, sc, R.x, R.p, R.r, R.n);
    return MGCG_HIP(hipGetLastError());
}

bool block_enqueue_start(const BlockRun& R) { return dispatch_k(R.k, [&](auto K) { return block_enqueue_start_k<K.value>(R); }); }
bool block_enqueue_iteration(const BlockRun& R, const FinalizeArgs& f) { return dispatch_k(R.k, [&](auto K) { return block_enqueue_iteration_k<K.value>(R, f); }); }
void block_enqueue_snapshot(Workspace* ws, volatile int* slot) { hipLaunchKernelGGL(block_snapshot_kernel, dim3(1), dim3(1), 0, ws->stream, (const BlockScalars*)ws->blockScalars, slot); }

bool block_read_results(Workspace* ws, BlockResult* out)
{
    BlockScalars h;
    if (!MGCG_HIP(hipMemcpy(&h, ws->blockScalars, sizeof(h), hipMemcpyDeviceToHost))) return false;
    memcpy(out->iteration, h.iteration, sizeof(h.iteration)); memcpy(out->residual, h.residual, sizeof(h.residual)); memcpy(out->status, h.status, sizeof(h.status));
    return true;
}

template <int K>
static void csrmv_block(hipStream_t s, double* y, const double* elements, const int* rowOffsets, const int* columnIndeces, const double* x, int count)
{
    BlockSpmvArgs a{};
    a.elements = elements; a.rowOffsets = rowOffsets; a.columnIndeces = columnIndeces;
    a.x = x; a.y = y; a.ld = count; a.rows = count;
    (void)launch_spmv_block<K>(s, BEPI_PLAIN, a, count >= 8000000);
}

void launch_spmv_block_plain(hipStream_t s, int k, const double* elements, const int* rowOffsets, const int* columnIndeces,
                             const double* x, double* y, long long ld, long long rows, const int* done)
{
    if (rows <= 0) return;
    BlockSpmvArgs a{};
    a.elements = elements; a.rowOffsets = rowOffsets; a.columnIndeces = columnIndeces;
    a.x = x; a.y = y; a.ld = ld; a.rows = (int)rows; a.done = done;
    dispatch_k(k, [&](auto K) { (void)launch_spmv_block<K.value>(s, BEPI_PLAIN, a, rows >= 8000000); });
}

void preload_kernels_block() { preload_code_object(reinterpret_cast<const void*>(&block_snapshot_kernel)); }

} // namespace mgcg

using namespace mgcg;

extern "C" {

void CsrMVBlock(MgcgSparse* cusparse, MgcgMatDescr* matDescr, double* y, const double* elements, const int* rowOffsets,
                const int* columnIndeces, const double* x, int elementsCount, int count, int k)
{
    (void)matDescr;
    if (!device_state()) return;
    if (!cusparse || !y || !rowOffsets || !x || (elementsCount > 0 && (!elements || !columnIndeces))) { set_error("CsrMVBlock: null argument"); return; }
    if (k < 1 || k > kBlockMaxK) { set_error("CsrMVBlock: k = %d columns, must be 1 .. %d", k, kBlockMaxK); return; }
    if (count < 0 || elementsCount < 0) { set_error("CsrMVBlock: negative size"); return; }
    if (count == 0) return;
    analysis_note_write(y, sizeof(double) * (size_t)k * (size_t)count);
    hipStream_t s = cusparse->ws.stream;
    dispatch_k(k, [&](auto K) { csrmv_block<K.value>(s, y, elements, rowOffsets, columnIndeces, x, count); });
    (void)MGCG_HIP(hipGetLastError());
}

} // extern "C"
