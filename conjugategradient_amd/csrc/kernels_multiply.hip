// The CSR matrix product C = A B on the device (gfx950): the kernels of MgcgCsrMultiply.
// The contract is written out in include/MgcgGpu.h; tests/test_multiply_host.py states it in numpy and the kernels here must EQUAL it in
// every run.  The products of row i of C are numbered t = 0, 1, 2, ... (row i of A in stored order; per entry, the row of B it points to
// in stored order); c_ij is the serial sum, from +0.0 and in ascending t, of the products that land on column j.  No float atomics; the
// integer atomics below count, take a minimum or maximum, or hand out slots of a work list whose order changes nothing.
//   columns:   every stored column lies in [0, bound) (the smallest offending row by atomicMin, as the transposition's count pass does)
//   products:  one lane per row: u_i = the sum over row i of A of the lengths of the rows of B it points to (64-bit; a row beyond INT_MAX
//              is flagged).  The rows above the register class go into a work list; the largest u of all is kept.
//   one pass, run twice: COUNT gives the stored entries of every row of C (exclusive_scan then gives C's offsets and the count of C, so
//              every refusal is made before anything is written), FILL writes the columns and the values.  Nothing is kept between the
//              two but the offsets: no array of all products exists.  Three classes by u_i:
//                u <= kMultiplyShortMax = 32:   one lane, columns and products in registers (8 wide, or 32): a product opens an entry of C
//                                               when no earlier one has its column; its place is the number of opening products with a
//                                               smaller column; its value is the sum over the later products of the same column, in order
//                u <= kMultiplyLdsMax = 2048:   one workgroup, expand - sort - compress in LDS: the keys (column << 32) | t are sorted by
//                                               a bitonic network; the lane at a run's first key sums the run serially -- ascending t --
//                                               from the products stored by t.  64 lanes (one wavefront) up to kMultiplyWaveMax = 256
//                                               products, kBlock lanes beyond.
//                anything longer:               one workgroup of kMultiplyLongBlock lanes, the same in global scratch of the library's own
//                                               (slow: log^2 passes over the row; no limit but INT_MAX and the memory)
//              The expansion takes the row of A in chunks of one entry a lane: a scan of the chunk's B-row lengths in LDS, and every lane
//              finds the entry of its products by bisection -- rows of A and of B of any length, empty ones included, share the lanes evenly.
#include "common.hpp"

namespace mgcg {

typedef unsigned long long MultiplyKey;
constexpr int kMultiplyWave = 64;              // lanes of the workgroup (one wavefront) for rows of kMultiplyWaveMax products or fewer
constexpr int kMultiplyWaveMax = 256;
constexpr int kMultiplyLongBlock = 1024;       // lanes of the one workgroup that works on a row in global memory

static inline int multiply_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// the row that stores position k: the largest i < rows with offsets[i] <= k (offsets checked: 0 = offsets[0] <= ... <= offsets[rows], k < offsets[rows])
__device__ __forceinline__ int multiply_row_of(const int* __restrict__ offsets, long long rows, long long k)
{
    long long lo = 0, hi = rows;                   // offsets[lo] <= k < offsets[hi]
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    return (int)lo;
}

// ---------------------------------------------------------------- checks and the products of every row
// *badRow (pre-set to INT_MAX) = the smallest row that stores a column outside [0, bound)
__global__ __launch_bounds__(kBlock) void multiply_check_columns_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long rows,
                                                                        long long bound, long long nnz, int* badRow)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
        const int c = columnIndeces[k];
        if (c < 0 || c >= bound) atomicMin(badRow, multiply_row_of(rowOffsets, rows, k));
    }
}
void launch_multiply_check_columns(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long bound, long long nnz, int* badRow)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(multiply_check_columns_kernel, dim3(multiply_grid(nnz)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, rows, bound, nnz, badRow);
}

// products[i] = u_i; stat2[0] (pre-set to INT_MAX) = the smallest row with u_i above INT_MAX, stat2[1] (pre-set to 0) = the largest u_i;
// work[0] (zeroed) counts the rows above the register class and work[1 ..] holds them.  Both matrices have passed their checks.
__global__ __launch_bounds__(kBlock) void multiply_products_kernel(const int* __restrict__ rowOffsetsA, const int* __restrict__ columnIndecesA,
                                                                   const int* __restrict__ rowOffsetsB, long long rows, int* __restrict__ products, int* work, int* stat2)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        long long u = 0;
        for (int p = rowOffsetsA[i], end = rowOffsetsA[i + 1]; p < end; ++p) {
            const int k = columnIndecesA[p];
            u += rowOffsetsB[k + 1] - rowOffsetsB[k];
        }
        if (u > 0x7fffffffLL) { atomicMin(&stat2[0], (int)i); products[i] = 0; continue; }
        products[i] = (int)u;
        if (u > kMultiplyShortMax) {
            work[1 + atomicAdd(&work[0], 1)] = (int)i;
            atomicMax(&stat2[1], (int)u);
        }
    }
}
void launch_multiply_products(hipStream_t s, const int* rowOffsetsA, const int* columnIndecesA, const int* rowOffsetsB, long long rows, int* products, int* work, int* stat2)
{
    hipLaunchKernelGGL(multiply_products_kernel, dim3(multiply_grid(rows)), dim3(kBlock), 0, s, rowOffsetsA, columnIndecesA, rowOffsetsB, rows, products, work, stat2);
}

// *total (zeroed) = the sum of lengths[0 .. rows) in 64 bits
__global__ __launch_bounds__(kBlock) void multiply_total_kernel(const int* __restrict__ lengths, long long rows, unsigned long long* total)
{
    const long long stride = (long long)gridDim.x * kBlock;
    unsigned long long sum = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) sum += (unsigned long long)lengths[i];
    if (sum != 0) atomicAdd(total, sum);
}
void launch_multiply_total(hipStream_t s, const int* lengths, long long rows, unsigned long long* total)
{
    hipLaunchKernelGGL(multiply_total_kernel, dim3(multiply_grid(rows)), dim3(kBlock), 0, s, lengths, rows, total);
}

// ---------------------------------------------------------------- the register class
// The n <= W products of one row, by one lane.  Static indexing throughout, so columns and products live in registers; -1 pads (no column
// equals it).  Returns the stored entries of the row of C; FILL writes them to outCols / outVals (the row's first entry; outVals may be null).
template <int W, bool FILL>
__device__ __forceinline__ int multiply_row_registers(const MultiplyArgs& a, int pBegin, int n, int* __restrict__ outCols, double* __restrict__ outVals)
{
    const bool values = FILL && a.elementsA != nullptr;
    int col[W];
    double prod[W];
    int p = pBegin - 1, q = 0, qEnd = 0;
    double av = 0.0;
#pragma unroll
    for (int t = 0; t < W; ++t) {
        col[t] = -1;
        prod[t] = 0.0;
        if (t < n) {
            while (q == qEnd) {                    // the next entry of A whose row of B is not empty: there is one, n counts these products
                ++p;
                const int k = a.columnIndecesA[p];
                q = a.rowOffsetsB[k];
                qEnd = a.rowOffsetsB[k + 1];
                if (values) av = a.elementsA[p];
            }
            col[t] = a.columnIndecesB[q];
            if (values) prod[t] = av * a.elementsB[q];
            ++q;
        }
    }
    unsigned opens = 0;                            // bit t: product t is the first of its column
#pragma unroll
    for (int t = 0; t < W; ++t) {
        bool first = t < n;
#pragma unroll
        for (int s = 0; s < t; ++s) first = first && col[s] != col[t];
        if (first) opens |= 1u << t;
    }
    if (!FILL) return __popc(opens);
#pragma unroll
    for (int t = 0; t < W; ++t) {
        if ((opens >> t) & 1u) {
            int rank = 0;
            double acc = 0.0;
#pragma unroll
            for (int s = 0; s < W; ++s) {
                rank += (((opens >> s) & 1u) != 0 && col[s] < col[t]) ? 1 : 0;
                if (s >= t && col[s] == col[t]) acc = acc + prod[s];
            }
            outCols[rank] = col[t];
            if (values) outVals[rank] = acc;
        }
    }
    return __popc(opens);
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void multiply_short_kernel(const MultiplyArgs a)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.rows; i += stride) {
        const int n = a.products[i];
        if (n > kMultiplyShortMax) continue;
        int count = 0;
        if (n > 0) {
            const int pBegin = a.rowOffsetsA[i];
            int* outCols = FILL ? a.outColumnIndeces + a.offsetsC[i] : nullptr;
            double* outVals = FILL && a.outElements != nullptr ? a.outElements + a.offsetsC[i] : nullptr;
            if (n <= 8) count = multiply_row_registers<8, FILL>(a, pBegin, n, outCols, outVals);
            else count = multiply_row_registers<kMultiplyShortMax, FILL>(a, pBegin, n, outCols, outVals);
        }
        if (!FILL) a.lengths[i] = count;
    }
}

// ---------------------------------------------------------------- the workgroup classes
// The inclusive scan of one int a lane over the workgroup, left in s_incl (read it after the call; a __syncthreads before the next one)
template <int THREADS>
__device__ __forceinline__ void multiply_scan(int* s_incl, int v)
{
    const int tid = (int)threadIdx.x;
    s_incl[tid] = v;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const int add = tid >= off ? s_incl[tid - off] : 0;
        __syncthreads();
        s_incl[tid] += add;
        __syncthreads();
    }
}

// The bitonic network of kernels_transpose.hip: every comparison points the same way (the first step of a merge mirrors: partner =
// i ^ (k - 1); the later ones are i | j), so the smaller key always goes to the smaller index and the positions from len up to the next
// power of two never take part: any length sorts in place.  a: LDS or global memory.
template <int THREADS>
__device__ __forceinline__ void multiply_sort_network(MultiplyKey* a, long long len)
{
    for (long long k = 2; (k >> 1) < len; k <<= 1) {
        for (long long j = k >> 1; j > 0; j >>= 1) {
            const long long pairs = ((len + 2 * j - 1) / (2 * j)) * j;                            // the pairs of the blocks of 2 j that hold a key
            for (long long t = threadIdx.x; t < pairs; t += THREADS) {
                const long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1));                        // bit j of i is clear
                const long long p = j == (k >> 1) ? (i ^ (k - 1)) : (i | j);
                if (p < len) {
                    const MultiplyKey x = a[i], y = a[p];
                    if (y < x) { a[i] = y; a[p] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// LDS that the row routine needs whatever holds the keys
template <int THREADS>
struct MultiplyShared {
    int incl[THREADS];         // the scan
    int firstB[THREADS];       // where the row of B of the chunk's entry begins
    double valueA[THREADS];    // the entry's value
    int count;
};

// One row of n products (n >= 1, and n <= the room of keys / prod) by the whole workgroup; every lane takes the same path.  COUNT: returns
// the stored entries of the row of C (to every lane).  FILL: writes them to outCols / outVals (outVals null: the pattern alone) and returns 0.
template <int THREADS, bool FILL>
__device__ __forceinline__ int multiply_row_workgroup(const MultiplyArgs& a, MultiplyShared<THREADS>& sh, MultiplyKey* keys, double* prod, int pBegin, int pEnd, int n,
                                                      int* __restrict__ outCols, double* __restrict__ outVals)
{
    const int tid = (int)threadIdx.x;
    const bool values = FILL && a.elementsA != nullptr;
    // expand: keys[t] = (column << 32) | t and prod[t], t in the order of the contract
    long long running = 0;
    for (long long base = pBegin; base < pEnd; base += THREADS) {
        const long long p = base + tid;
        int len = 0;
        if (p < pEnd) {
            const int k = a.columnIndecesA[p];
            const int begin = a.rowOffsetsB[k];
            len = a.rowOffsetsB[k + 1] - begin;
            sh.firstB[tid] = begin;
            if (values) sh.valueA[tid] = a.elementsA[p];
        }
        multiply_scan<THREADS>(sh.incl, len);
        const long long total = sh.incl[THREADS - 1];
        for (long long x = tid; x < total; x += THREADS) {
            int lo = 0, hi = THREADS - 1;                                   // the smallest m with incl[m] > x (incl[THREADS - 1] = total > x); its row of B is not empty
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sh.incl[mid] > x) hi = mid; else lo = mid + 1;
            }
            const long long q = sh.firstB[lo] + (x - (lo > 0 ? sh.incl[lo - 1] : 0));
            const long long t = running + x;                                // < n: the chunks' totals sum to n
            keys[t] = ((MultiplyKey)(unsigned)a.columnIndecesB[q] << 32) | (MultiplyKey)t;
            if (values) prod[t] = sh.valueA[lo] * a.elementsB[q];
        }
        running += total;
        __syncthreads();
    }
    multiply_sort_network<THREADS>(keys, n);
    if (!FILL) {
        if (tid == 0) sh.count = 0;
        __syncthreads();
        int mine = 0;
        for (long long x = tid; x < n; x += THREADS) mine += (x == 0 || (keys[x] >> 32) != (keys[x - 1] >> 32)) ? 1 : 0;
        if (mine) atomicAdd(&sh.count, mine);
        __syncthreads();
        const int count = sh.count;
        __syncthreads();
        return count;
    }
    // compress: the lane at a run's first key owns the entry; its place = the runs before it
    running = 0;
    for (long long base = 0; base < n; base += THREADS) {
        const long long x = base + tid;
        const bool first = x < n && (x == 0 || (keys[x] >> 32) != (keys[x - 1] >> 32));
        multiply_scan<THREADS>(sh.incl, first ? 1 : 0);
        if (first) {
            const long long place = running + sh.incl[tid] - 1;
            const MultiplyKey column = keys[x] >> 32;
            outCols[place] = (int)column;
            if (values) {
                double acc = 0.0;
                for (long long y = x; y < n && (keys[y] >> 32) == column; ++y) acc = acc + prod[keys[y] & 0xffffffffULL];
                outVals[place] = acc;
            }
        }
        running += sh.incl[THREADS - 1];
        __syncthreads();
    }
    return 0;
}

// the rows of the work list with LOW < u <= CAP, keys and products in LDS
template <int THREADS, int LOW, int CAP, bool FILL>
__global__ __launch_bounds__(THREADS) void multiply_lds_kernel(const MultiplyArgs a)
{
    __shared__ MultiplyKey s_key[CAP];
    __shared__ double s_prod[FILL ? CAP : 1];
    __shared__ MultiplyShared<THREADS> sh;
    const int listed = a.work[0];
    for (int w = (int)blockIdx.x; w < listed; w += (int)gridDim.x) {
        const int i = a.work[1 + w];
        const int n = a.products[i];
        if (n <= LOW || n > CAP) continue;                                  // (the same for every lane of the workgroup)
        int* outCols = FILL ? a.outColumnIndeces + a.offsetsC[i] : nullptr;
        double* outVals = FILL && a.outElements != nullptr ? a.outElements + a.offsetsC[i] : nullptr;
        const int count = multiply_row_workgroup<THREADS, FILL>(a, sh, s_key, s_prod, a.rowOffsetsA[i], a.rowOffsetsA[i + 1], n, outCols, outVals);
        if (!FILL && threadIdx.x == 0) a.lengths[i] = count;
        __syncthreads();
    }
}

// the rows of the work list with u > kMultiplyLdsMax, keys and products in the workgroup's segment of the scratch (scratchStride entries each)
template <bool FILL>
__global__ __launch_bounds__(kMultiplyLongBlock) void multiply_global_kernel(const MultiplyArgs a)
{
    __shared__ MultiplyShared<kMultiplyLongBlock> sh;
    MultiplyKey* keys = a.scratchKeys + (long long)blockIdx.x * a.scratchStride;
    double* prod = FILL && a.scratchProducts != nullptr ? a.scratchProducts + (long long)blockIdx.x * a.scratchStride : nullptr;
    const int listed = a.work[0];
    for (int w = (int)blockIdx.x; w < listed; w += (int)gridDim.x) {
        const int i = a.work[1 + w];
        const int n = a.products[i];
        if (n <= kMultiplyLdsMax || n > a.scratchStride) continue;
        int* outCols = FILL ? a.outColumnIndeces + a.offsetsC[i] : nullptr;
        double* outVals = FILL && a.outElements != nullptr ? a.outElements + a.offsetsC[i] : nullptr;
        const int count = multiply_row_workgroup<kMultiplyLongBlock, FILL>(a, sh, keys, prod, a.rowOffsetsA[i], a.rowOffsetsA[i + 1], n, outCols, outVals);
        if (!FILL && threadIdx.x == 0) a.lengths[i] = count;
        __syncthreads();                                                    // (orders the workgroup's global accesses before the segment is used again)
    }
}

template <bool FILL>
static void launch_multiply_pass_of(hipStream_t s, const MultiplyArgs& a, int listed, int longest, int longGrid)
{
    hipLaunchKernelGGL(multiply_short_kernel<FILL>, dim3(multiply_grid(a.rows)), dim3(kBlock), 0, s, a);
    if (listed <= 0) return;
    const int grid = listed < kMaxGrid ? listed : kMaxGrid;
    hipLaunchKernelGGL((multiply_lds_kernel<kMultiplyWave, kMultiplyShortMax, kMultiplyWaveMax, FILL>), dim3(grid), dim3(kMultiplyWave), 0, s, a);
    if (longest > kMultiplyWaveMax) hipLaunchKernelGGL((multiply_lds_kernel<kBlock, kMultiplyWaveMax, kMultiplyLdsMax, FILL>), dim3(grid), dim3(kBlock), 0, s, a);
    if (longest > kMultiplyLdsMax) hipLaunchKernelGGL(multiply_global_kernel<FILL>, dim3(longGrid), dim3(kMultiplyLongBlock), 0, s, a);
}

// One pass over every row of C.  fill false: a.lengths[i] = the stored entries of row i.  fill true: the columns and (a.outElements given)
// the values at a.offsetsC.  listed, longest: work[0] and stat2[1] of the products pass; longGrid workgroups share a.scratchKeys /
// a.scratchProducts, a.scratchStride >= longest entries each (needed only when longest > kMultiplyLdsMax).
bool launch_multiply_pass(hipStream_t s, const MultiplyArgs& a, bool fill, int listed, int longest, int longGrid)
{
    if (fill) launch_multiply_pass_of<true>(s, a, listed, longest, longGrid);
    else launch_multiply_pass_of<false>(s, a, listed, longest, longGrid);
    return MGCG_HIP(hipGetLastError());
}

void preload_kernels_multiply() { preload_code_object(reinterpret_cast<const void*>(&multiply_total_kernel)); }

} // namespace mgcg
