// Aggregation multigrid (gfx950): the indexed transfer of the V-cycle and the set-up kernels of MgSetupAggregation / MgSetupAggregates.
// The algorithm is written out in include/MgcgGpu.h; tests/test_amg_host.py states it in numpy and the kernels here must EQUAL it:
// every sum below is a serial sum in a fixed order from +0.0 (the library is built with -ffp-contract=off).
//   cycle:   amg_restrict_kernel (bc[I] = sum of r over I's members, ascending), amg_prolong_add_kernel (x[i] += e[agg[i]])
//   set-up:  the matching pass (row maxima, pick, match), the Galerkin product sigma * P^T A P for an arbitrary map, the diagonal check,
//            the value gather of the merged matrix [A | A^T] from which MgcgSymmetricPart's S = (A + A^T) / 2 is summed by the Galerkin product
#include "common.hpp"

namespace mgcg {

static inline int amg_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- the cycle
// bc[I] = ((0 + r[m0]) + r[m1]) + ...: one lane per aggregate, its members (at most 16, ascending) through the inverted index.  A gather of
// r by nature; with box aggregates in lexicographic order neighbouring lanes read neighbouring pairs, as restrict_kernel does.
__global__ __launch_bounds__(kBlock) void amg_restrict_kernel(long long nc, const int* __restrict__ aggOffsets, const int* __restrict__ members,
                                                              const double* __restrict__ r, double* __restrict__ bc, const int* done)
{
    if (done != nullptr && *done != 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long I = (long long)blockIdx.x * kBlock + threadIdx.x; I < nc; I += stride) {
        const int k0 = aggOffsets[I], k1 = aggOffsets[I + 1];
        double sum = 0.0;
        for (int k = k0; k < k1; ++k) sum += r[members[k]];
        bc[I] = sum;
    }
}
void launch_amg_restrict(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const double* r, double* bc, const int* done)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(amg_restrict_kernel, dim3(amg_grid(nc)), dim3(kBlock), 0, s, nc, aggOffsets, members, r, bc, done);
}

// x[i] += e[agg[i]]: x and agg stream (20 bytes per row), e is gathered (1/8 of the rows with the default aggregates: cache resident per wave)
__global__ __launch_bounds__(kBlock) void amg_prolong_add_kernel(long long n, const int* __restrict__ agg, double* __restrict__ x,
                                                                 const double* __restrict__ e, const int* done)
{
    if (done != nullptr && *done != 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] = x[i] + e[agg[i]];
}
void launch_amg_prolong_add(hipStream_t s, long long n, const int* agg, double* x, const double* e, const int* done)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(amg_prolong_add_kernel, dim3(amg_grid(n)), dim3(kBlock), 0, s, n, agg, x, e, done);
}

// ---------------------------------------------------------------- set-up: the diagonal
// *badRow = the smallest row whose diagonal (the first stored entry of column i, as extract_dinv_kernel reads it) is missing, not finite or
// not positive; pre-set to INT_MAX by the caller
__global__ __launch_bounds__(kBlock) void amg_check_diagonal_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets,
                                                                    const int* __restrict__ columnIndeces, long long n, int* badRow)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double d = 0.0;
        for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k)
            if (columnIndeces[k] == i) { d = elements[k]; break; }
        if (!(d > 0.0) || !(d <= 1.79769313486231570e308)) atomicMin(badRow, (int)i);
    }
}
void launch_amg_check_diagonal(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, int* badRow)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(amg_check_diagonal_kernel, dim3(amg_grid(n)), dim3(kBlock), 0, s, elements, rowOffsets, columnIndeces, n, badRow);
}

// ---------------------------------------------------------------- set-up: one matching pass
// rowMax[i] = the largest w = -value over the stored entries of row i with column != i and value < 0; 0 if there is none
__global__ __launch_bounds__(kBlock) void amg_row_max_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets,
                                                             const int* __restrict__ columnIndeces, long long n, double* __restrict__ rowMax)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double m = 0.0;
        for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
            const double v = elements[k];
            if (columnIndeces[k] != i && v < 0.0 && -v > m) m = -v;
        }
        rowMax[i] = m;
    }
}

// the symmetric tie-break key of edge {i, j}, 32-bit unsigned arithmetic
__device__ __forceinline__ unsigned amg_edge_key(unsigned i, unsigned j)
{
    const unsigned lo = i < j ? i : j, hi = i < j ? j : i;
    unsigned h = lo * 0x9E3779B1u + hi * 0x85EBCA77u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

// One round, first half: every unmatched row picks the neighbour with the largest (w, h, j) among its candidate edges (w >= theta m_i and
// w >= theta m_j, w from row i) whose other end is unmatched; pick[i] = -1 if it has none.  flags[0] = 1 if some row picked.
// match[] is read only (written by amg_match_kernel of the round before): no lane depends on another lane of this launch.
__global__ __launch_bounds__(kBlock) void amg_pick_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets,
                                                          const int* __restrict__ columnIndeces, long long n, double theta,
                                                          const double* __restrict__ rowMax, const int* __restrict__ match, int* __restrict__ pick, int* flags)
{
    bool any = false;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int best = -1;
        if (match[i] < 0) {
            const double ti = theta * rowMax[i];
            double bw = 0.0; unsigned bh = 0u;
            for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
                const int j = columnIndeces[k];
                const double v = elements[k];
                if (j == i || !(v < 0.0) || j < 0 || j >= n) continue;
                const double w = -v;
                if (!(w >= ti)) continue;
                const double tj = theta * rowMax[j];
                if (!(w >= tj) || match[j] >= 0) continue;
                const unsigned h = amg_edge_key((unsigned)i, (unsigned)j);
                const bool larger = best < 0 || w > bw || (w == bw && (h > bh || (h == bh && j > best)));
                if (larger) { best = j; bw = w; bh = h; }
            }
        }
        pick[i] = best;
        any = any || best >= 0;
    }
    if (any) flags[0] = 1;
}
// second half: rows that picked each other are matched.  pick[] is read only, a lane writes its own match[i].  flags[1] = 1 if some pair formed.
__global__ __launch_bounds__(kBlock) void amg_match_kernel(long long n, const int* __restrict__ pick, int* __restrict__ match, int* flags)
{
    bool any = false;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int j = pick[i];
        if (j >= 0 && pick[j] == (int)i) { match[i] = j; any = true; }
    }
    if (any) flags[1] = 1;
}
void launch_amg_row_max(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, double* rowMax)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(amg_row_max_kernel, dim3(amg_grid(n)), dim3(kBlock), 0, s, elements, rowOffsets, columnIndeces, n, rowMax);
}
void launch_amg_match_round(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, double theta,
                            const double* rowMax, int* match, int* pick, int* flags2)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(amg_pick_kernel, dim3(amg_grid(n)), dim3(kBlock), 0, s, elements, rowOffsets, columnIndeces, n, theta, rowMax, match, pick, flags2);
    hipLaunchKernelGGL(amg_match_kernel, dim3(amg_grid(n)), dim3(kBlock), 0, s, n, pick, match, flags2);
}

// ---------------------------------------------------------------- set-up: sigma * P^T A P for an arbitrary map
// One lane per coarse row I.  Its fine entries in the contract's order -- members ascending, each member's entries in stored order -- number
// expandOffsets[I + 1] - expandOffsets[I]; the lane owns that many ints of `scratch` from expandOffsets[I] on.
// Count pass: the coarse column of every entry goes to the lane's scratch, is sorted there (heap sort, in place) and made unique; the unique
// columns stay at the front of the segment for the fill pass.  counts[I] = how many.
__device__ inline void amg_sift_down(int* a, int start, int end)
{
    int root = start;
    for (;;) {
        int child = 2 * root + 1;
        if (child >= end) return;
        if (child + 1 < end && a[child] < a[child + 1]) ++child;
        if (a[root] >= a[child]) return;
        const int t = a[root]; a[root] = a[child]; a[child] = t;
        root = child;
    }
}
__global__ __launch_bounds__(kBlock) void amg_galerkin_count_kernel(long long nc, const int* __restrict__ aggOffsets, const int* __restrict__ members,
                                                                    const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                                    const int* __restrict__ agg, const int* __restrict__ expandOffsets,
                                                                    int* __restrict__ scratch, int* __restrict__ counts)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long I = (long long)blockIdx.x * kBlock + threadIdx.x; I < nc; I += stride) {
        int* seg = scratch + expandOffsets[I];
        const int len = expandOffsets[I + 1] - expandOffsets[I];
        int at = 0;
        for (int m = aggOffsets[I]; m < aggOffsets[I + 1]; ++m) {
            const int i = members[m];
            for (int k = rowOffsets[i]; k < rowOffsets[i + 1] && at < len; ++k) seg[at++] = agg[columnIndeces[k]];
        }
        for (int start = at / 2 - 1; start >= 0; --start) amg_sift_down(seg, start, at);
        for (int end = at - 1; end > 0; --end) {
            const int t = seg[0]; seg[0] = seg[end]; seg[end] = t;
            amg_sift_down(seg, 0, end);
        }
        int u = 0;
        for (int k = 0; k < at; ++k)
            if (u == 0 || seg[k] != seg[u - 1]) seg[u++] = seg[k];
        counts[I] = u;
    }
}
// Fill pass: the unique columns become the coarse row's column ids (ascending), every accumulator starts at +0.0, then every fine value is
// added to the accumulator of its coarse column in the contract's order (the lane is the only one that touches its row: a serial sum), and
// each accumulator is scaled once: sigma * acc.
__global__ __launch_bounds__(kBlock) void amg_galerkin_fill_kernel(long long nc, const int* __restrict__ aggOffsets, const int* __restrict__ members,
                                                                   const double* __restrict__ elements, const int* __restrict__ rowOffsets,
                                                                   const int* __restrict__ columnIndeces, const int* __restrict__ agg,
                                                                   const int* __restrict__ expandOffsets, const int* __restrict__ scratch,
                                                                   const int* __restrict__ rowOffsetsC, double sigma,
                                                                   double* __restrict__ elementsC, int* __restrict__ columnIndecesC)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long I = (long long)blockIdx.x * kBlock + threadIdx.x; I < nc; I += stride) {
        const int* seg = scratch + expandOffsets[I];
        const int base = rowOffsetsC[I], u = rowOffsetsC[I + 1] - base;
        if (u <= 0) continue;
        int* cols = columnIndecesC + base;
        double* acc = elementsC + base;
        for (int q = 0; q < u; ++q) { cols[q] = seg[q]; acc[q] = 0.0; }
        for (int m = aggOffsets[I]; m < aggOffsets[I + 1]; ++m) {
            const int i = members[m];
            for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
                const int J = agg[columnIndeces[k]];
                int lo = 0, hi = u - 1;                     // J is among the u columns: the count pass put it there
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg[mid] < J) lo = mid + 1; else hi = mid; }
                acc[lo] = acc[lo] + elements[k];
            }
        }
        for (int q = 0; q < u; ++q) acc[q] = sigma * acc[q];
    }
}
void launch_amg_galerkin_count(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                               const int* agg, const int* expandOffsets, int* scratch, int* counts)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(amg_galerkin_count_kernel, dim3(amg_grid(nc)), dim3(kBlock), 0, s, nc, aggOffsets, members, rowOffsets, columnIndeces, agg, expandOffsets, scratch, counts);
}
void launch_amg_galerkin_fill(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const double* elements, const int* rowOffsets,
                              const int* columnIndeces, const int* agg, const int* expandOffsets, const int* scratch, const int* rowOffsetsC, double sigma,
                              double* elementsC, int* columnIndecesC)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(amg_galerkin_fill_kernel, dim3(amg_grid(nc)), dim3(kBlock), 0, s, nc, aggOffsets, members, elements, rowOffsets, columnIndeces, agg, expandOffsets,
                       scratch, rowOffsetsC, sigma, elementsC, columnIndecesC);
}

// ---------------------------------------------------------------- the symmetric part: the values of [A | A^T] row by row
// out[k] = elements[source[k]]: `source` is the host-built list of A's entries in the order of the merged matrix (row i of A in stored order,
// then the entries of column i by source row and stored order: the transposition permutation).  One lane per merged entry; out streams,
// the A half of every row reads a contiguous run, the A^T half is the gather a transposition is.
__global__ __launch_bounds__(kBlock) void amg_gather_values_kernel(long long m, const int* __restrict__ source, const double* __restrict__ elements,
                                                                   double* __restrict__ out)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < m; k += stride) out[k] = elements[source[k]];
}
void launch_amg_gather_values(hipStream_t s, long long m, const int* source, const double* elements, double* out)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(amg_gather_values_kernel, dim3(amg_grid(m)), dim3(kBlock), 0, s, m, source, elements, out);
}

void preload_kernels_amg() { preload_code_object(reinterpret_cast<const void*>(&amg_restrict_kernel)); }

} // namespace mgcg
