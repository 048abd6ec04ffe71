// Numeric refresh of an aggregation hierarchy (gfx950; MgUpdateValues): new values for a pattern whose maps are kept.
// The contract is written out in include/MgcgGpu.h; tests/test_refresh_host.py states it in numpy and the kernels here must EQUAL it.
//   once per hierarchy:  the source list of every Galerkin product -- per coarse entry q the stored positions of the fine entries behind it,
//                        in the contract's order (members ascending, each member's entries in stored order); no value is read
//   per refresh:         C[q] = sigma * (((+0.0 + a[src[o]]) + a[src[o + 1]]) + ...): one streaming pass over the list, the serial sum of a
//                        segment by ONE lane (the library is built with -ffp-contract=off)
#include "common.hpp"

namespace mgcg {

static inline int refresh_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- the source lists
// One lane per coarse row I: the walk of amg_galerkin_fill_kernel -- members ascending, each member's entries in stored order, the coarse
// column J found among the row's u ascending columns by bisection -- with a cursor per coarse entry where that kernel has an accumulator.
// The lane is the only one that touches its row's counters, and it meets the entries of a coarse entry in the contract's order: the
// grouping is a stable counting sort.  Neighbouring entries mostly fall into one coarse entry (an aggregate of everything: all of them),
// so the counter of the run in hand lives in a register and goes to memory when the coarse entry changes.
// Fill = false: slots[q] += the entries behind q (slots zeroed by the caller: nnz(C) + 1 ints, scanned into the segment offsets afterwards).
// Fill = true:  slots[q] = where q's next source goes (a copy of the offsets); sources[...] = the stored position k.  A position at or
//               beyond `held` is not written (the offsets the caller promised unchanged would have to have grown).
template <bool Fill>
__global__ __launch_bounds__(kBlock) void refresh_sources_kernel(long long nc, const int* __restrict__ aggOffsets, const int* __restrict__ members,
                                                                 const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                                 const int* __restrict__ agg, const int* __restrict__ rowOffsetsC,
                                                                 const int* __restrict__ columnIndecesC, int* __restrict__ slots, long long held,
                                                                 int* __restrict__ sources)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long I = (long long)blockIdx.x * kBlock + threadIdx.x; I < nc; I += stride) {
        const int base = rowOffsetsC[I], u = rowOffsetsC[I + 1] - base;
        if (u <= 0) continue;
        const int* cols = columnIndecesC + base;
        int* slot = slots + base;
        int at = -1, lastJ = -1, run = 0;                   // the coarse entry in hand: its place in the row, its column, its counter
        for (int m = aggOffsets[I]; m < aggOffsets[I + 1]; ++m) {
            const int i = members[m];
            for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
                const int J = agg[columnIndeces[k]];
                if (at < 0 || J != lastJ) {
                    if (at >= 0) slot[at] = run;
                    int lo = 0, hi = u - 1;                 // J is among the u columns: the set-up's count pass put it there
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cols[mid] < J) lo = mid + 1; else hi = mid; }
                    at = lo; lastJ = J; run = slot[at];
                }
                if (Fill) { if (run < held) sources[run] = k; }
                ++run;
            }
        }
        if (at >= 0) slot[at] = run;
    }
}
void launch_refresh_sources_count(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                                  const int* agg, const int* rowOffsetsC, const int* columnIndecesC, int* counts)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(refresh_sources_kernel<false>, dim3(refresh_grid(nc)), dim3(kBlock), 0, s, nc, aggOffsets, members, rowOffsets, columnIndeces, agg,
                       rowOffsetsC, columnIndecesC, counts, 0LL, (int*)nullptr);
}
void launch_refresh_sources_fill(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                                 const int* agg, const int* rowOffsetsC, const int* columnIndecesC, int* cursor, long long held, int* sources)
{
    if (nc <= 0) return;
    hipLaunchKernelGGL(refresh_sources_kernel<true>, dim3(refresh_grid(nc)), dim3(kBlock), 0, s, nc, aggOffsets, members, rowOffsets, columnIndeces, agg,
                       rowOffsetsC, columnIndecesC, cursor, held, sources);
}

// ---------------------------------------------------------------- the numeric pass
// The first q in [0, n] with offsets[q] >= x (offsets: n + 1 ints that never descend)
__device__ __forceinline__ int refresh_lower_bound(const int* __restrict__ offsets, long long n, long long x)
{
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (offsets[mid] < x) lo = mid + 1; else hi = mid; }
    return (int)lo;
}
// A workgroup takes the list in contiguous tiles of kRefreshTile sources: `sources` streams (coalesced), every value is gathered ONCE into
// LDS, and the segments whose HEAD lies in the tile -- a contiguous range of q, found by two bisections of the offsets -- go one to a lane,
// which adds its run serially from LDS in list order.  With 1.4 - 5.4 sources per segment on the measured hierarchies a tile feeds
// 380 - 1460 segments, two to six trips of the 256 lanes.  A segment that runs past the tile's end (at most one per tile does) goes on
// from global memory, through `sources`, in the same order: the same additions by the same lane, hence the same bits whatever the tile
// size and the grid.  An empty segment (the set-up makes none) would give sigma * +0.0.
// LDS: 16 KiB of values a workgroup, 8 resident workgroups per CU: 128 of the CU's 160 KiB.
__global__ __launch_bounds__(kBlock) void refresh_numeric_kernel(long long segments, long long sourceCount, const int* __restrict__ segmentOffsets,
                                                                 const int* __restrict__ sources, const double* __restrict__ elements, double sigma,
                                                                 double* __restrict__ elementsC)
{
    __shared__ double vals[kRefreshTile];
    __shared__ int range[2];
    const long long tiles = (sourceCount + kRefreshTile - 1) / kRefreshTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long base = t * kRefreshTile;
        const long long end = base + kRefreshTile < sourceCount ? base + kRefreshTile : sourceCount;
        const int len = (int)(end - base);
        for (int j = threadIdx.x; j < len; j += kBlock) vals[j] = elements[sources[base + j]];
        if (threadIdx.x == 0) range[0] = refresh_lower_bound(segmentOffsets, segments, base);
        if (threadIdx.x == 64) range[1] = t + 1 == tiles ? (int)segments : refresh_lower_bound(segmentOffsets, segments, end);
        __syncthreads();
        const int q1 = range[1];
        for (int q = range[0] + (int)threadIdx.x; q < q1; q += kBlock) {
            const long long o0 = segmentOffsets[q], o1 = segmentOffsets[q + 1];
            const long long staged = o1 < end ? o1 : end;
            double sum = 0.0;
            long long o = o0;
            for (; o < staged; ++o) sum = sum + vals[o - base];
            for (; o < o1; ++o) sum = sum + elements[sources[o]];
            elementsC[q] = sigma * sum;
        }
        __syncthreads();                                   // the next tile overwrites vals and range
    }
}
void launch_refresh_numeric(hipStream_t s, long long segments, long long sourceCount, const int* segmentOffsets, const int* sources, const double* elements,
                            double sigma, double* elementsC)
{
    if (segments <= 0 || sourceCount <= 0) return;
    long long tiles = (sourceCount + kRefreshTile - 1) / kRefreshTile;
    if (tiles > kMaxGrid) tiles = kMaxGrid;
    hipLaunchKernelGGL(refresh_numeric_kernel, dim3((int)tiles), dim3(kBlock), 0, s, segments, sourceCount, segmentOffsets, sources, elements, sigma, elementsC);
}

void preload_kernels_refresh() { preload_code_object(reinterpret_cast<const void*>(&refresh_numeric_kernel)); }

} // namespace mgcg
