// CSR transposition on the device (gfx950): the kernels of MgcgCsrTranspose and of the merged matrix [A | A^T] of MgcgSymmetricPart.
// The contract is written out in include/MgcgGpu.h; tests/test_transpose_host.py states it in numpy (a stable sort by column) and the
// kernels here must EQUAL it in every run.  No float atomics; the integer atomics below either add (counts: the sum does not depend on the
// order of arrival) or hand out slots whose order is then erased by a sort.
//   check:        the offsets start at 0, never descend (the smallest offending row through one atomicMin flag) and end at or below the count
//   count:        every stored column lies in [0, columns) (the smallest offending row, again by atomicMin); counts[c] = how often column c
//                 is stored = the length of row c of A^T (integer atomicAdd); exclusive_scan makes the offsets of A^T from them
//   claim:        entry k of A takes a slot of its column's segment by atomicAdd on a cursor and stores the 64-bit key (k << 32) | row there
//   canonicalise: every segment is sorted by its keys ascending.  k is A's stored position: it ascends with the row and, inside a row, with
//                 the stored order, so the one sort gives "source rows ascending, stored order within one row", duplicates included, and
//                 the slot order of the claim pass is gone.  Three width classes by the length of a segment:
//                   length <= kTransposeShortMax = 32:    one lane, a rank sort in registers (8 keys wide, or 32)
//                   length <= kTransposeLdsMax   = 4096:  one workgroup of kBlock lanes, a bitonic network in LDS (32 KiB)
//                   anything longer:                      one workgroup of kTransposeLongBlock lanes, the same network in global memory in
//                                                         place -- slow (log^2 passes over the segment by 1024 lanes) and without a length limit
//                 The one-lane pass writes the columns of the two upper classes into a work list (its order is arbitrary and changes
//                 nothing: every segment is sorted on its own); the two workgroup passes walk that list.
//   emit:         out column = the low word (the row of A), out source = the high word (k), out value = elements[k], a bit copy
//   merged:       offsets ro[i] + tro[i], and per row A's entries in stored order, then A^T's: columns and the source list
#include "common.hpp"

namespace mgcg {

typedef unsigned long long TransposeKey;
constexpr int kTransposeLongBlock = 1024;      // lanes of the one workgroup that sorts a segment in global memory
constexpr int kTransposeLongGrid = 256;        // workgroups that walk the work list for such segments

static inline int transpose_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// the row that stores position k: the largest i < rows with offsets[i] <= k (offsets checked: 0 = offsets[0] <= ... <= offsets[rows], k < offsets[rows])
__device__ __forceinline__ int transpose_row_of(const int* __restrict__ offsets, long long rows, long long k)
{
    long long lo = 0, hi = rows;                   // offsets[lo] <= k < offsets[hi]
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    return (int)lo;
}

// ---------------------------------------------------------------- check and count
// status[0] (pre-set to INT_MAX) = the smallest row i with rowOffsets[i + 1] < rowOffsets[i]; status[1] = rowOffsets[0]; status[2] = rowOffsets[rows]
__global__ __launch_bounds__(kBlock) void transpose_check_offsets_kernel(const int* __restrict__ rowOffsets, long long rows, int* status)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride)
        if (rowOffsets[i + 1] < rowOffsets[i]) atomicMin(status, (int)i);
    if (blockIdx.x == 0 && threadIdx.x == 0) { status[1] = rowOffsets[0]; status[2] = rowOffsets[rows]; }
}
void launch_transpose_check_offsets(hipStream_t s, const int* rowOffsets, long long rows, int* status3)
{
    hipLaunchKernelGGL(transpose_check_offsets_kernel, dim3(transpose_grid(rows)), dim3(kBlock), 0, s, rowOffsets, rows, status3);
}

// counts[c] += 1 for every stored column c in range (counts zeroed by the caller); *badRow (pre-set to INT_MAX) = the smallest row that stores a
// column outside [0, columns)
__global__ __launch_bounds__(kBlock) void transpose_count_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long rows,
                                                                 long long columns, long long nnz, int* counts, int* badRow)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
        const int c = columnIndeces[k];
        if (c < 0 || c >= columns) atomicMin(badRow, transpose_row_of(rowOffsets, rows, k));
        else atomicAdd(&counts[c], 1);
    }
}
void launch_transpose_count(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long columns, long long nnz, int* counts, int* badRow)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(transpose_count_kernel, dim3(transpose_grid(nnz)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, rows, columns, nnz, counts, badRow);
}

// ---------------------------------------------------------------- claim
// cursor[c] starts at the offset of A^T's row c; every column was found in range by the count pass
__global__ __launch_bounds__(kBlock) void transpose_claim_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long rows,
                                                                 long long nnz, int* cursor, TransposeKey* __restrict__ keys)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
        const int row = transpose_row_of(rowOffsets, rows, k);
        const int slot = atomicAdd(&cursor[columnIndeces[k]], 1);
        keys[slot] = ((TransposeKey)k << 32) | (TransposeKey)(unsigned)row;
    }
}

// ---------------------------------------------------------------- canonicalise
// len <= W keys of one lane's segment: every key's rank among them (they differ: k is unique), then each to its place.  Static indexing
// throughout, so the keys live in registers; ~0 pads (no key equals it: k < 2^31).
template <int W>
__device__ __forceinline__ void transpose_sort_registers(TransposeKey* __restrict__ seg, int len)
{
    TransposeKey key[W];
#pragma unroll
    for (int j = 0; j < W; ++j) key[j] = j < len ? seg[j] : ~0ULL;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) rank += key[j] < key[i] ? 1 : 0;
        if (i < len) seg[rank] = key[i];
    }
}

// one lane per column: the short segments are sorted, the others listed (work[0], zeroed by the caller, counts them; work[1 ..] holds them)
__global__ __launch_bounds__(kBlock) void transpose_sort_short_kernel(const int* __restrict__ offsetsT, long long columns, TransposeKey* __restrict__ keys, int* work)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < columns; c += stride) {
        const int begin = offsetsT[c], len = offsetsT[c + 1] - begin;
        if (len <= 1) continue;
        if (len <= 8) transpose_sort_registers<8>(keys + begin, len);
        else if (len <= kTransposeShortMax) transpose_sort_registers<kTransposeShortMax>(keys + begin, len);
        else work[1 + atomicAdd(&work[0], 1)] = (int)c;
    }
}

// The bitonic network with every comparison pointing the same way (the first step of a merge mirrors: partner = i ^ (k - 1); the later ones
// are i ^ j), so the smaller key always goes to the smaller index and the positions from len up to the next power of two, which would hold
// +infinity, never take part: any length sorts in place.  a: LDS or global memory; the workgroup's THREADS lanes share the pairs of a step.
template <int THREADS>
__device__ __forceinline__ void transpose_sort_network(TransposeKey* a, long long len)
{
    for (long long k = 2; (k >> 1) < len; k <<= 1) {
        for (long long j = k >> 1; j > 0; j >>= 1) {
            const long long pairs = ((len + 2 * j - 1) / (2 * j)) * j;                            // the pairs of the blocks of 2 j that hold a key
            for (long long t = threadIdx.x; t < pairs; t += THREADS) {
                const long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1));                        // bit j of i is clear
                const long long p = j == (k >> 1) ? (i ^ (k - 1)) : (i | j);
                if (p < len) {
                    const TransposeKey x = a[i], y = a[p];
                    if (y < x) { a[i] = y; a[p] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBlock) void transpose_sort_lds_kernel(const int* __restrict__ offsetsT, const int* __restrict__ work, TransposeKey* __restrict__ keys)
{
    __shared__ TransposeKey s_key[kTransposeLdsMax];
    const int listed = work[0];
    for (int w = (int)blockIdx.x; w < listed; w += (int)gridDim.x) {
        const int c = work[1 + w];
        const int begin = offsetsT[c], len = offsetsT[c + 1] - begin;
        if (len > kTransposeLdsMax) continue;                                       // (the same for every lane of the workgroup)
        for (int t = (int)threadIdx.x; t < len; t += kBlock) s_key[t] = keys[begin + t];
        __syncthreads();
        transpose_sort_network<kBlock>(s_key, len);
        for (int t = (int)threadIdx.x; t < len; t += kBlock) keys[begin + t] = s_key[t];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kTransposeLongBlock) void transpose_sort_global_kernel(const int* __restrict__ offsetsT, const int* __restrict__ work, TransposeKey* keys)
{
    const int listed = work[0];
    for (int w = (int)blockIdx.x; w < listed; w += (int)gridDim.x) {
        const int c = work[1 + w];
        const int begin = offsetsT[c], len = offsetsT[c + 1] - begin;
        if (len <= kTransposeLdsMax) continue;
        transpose_sort_network<kTransposeLongBlock>(keys + begin, len);             // (__syncthreads orders the workgroup's global accesses)
    }
}

// offsetsT: the offsets of A^T (columns + 1); cursor: columns ints of scratch; work: 1 + min(columns, nnz / (kTransposeShortMax + 1)) ints of scratch;
// keys: nnz.  Afterwards keys[offsetsT[c] .. offsetsT[c + 1]) are the entries of column c by ascending stored position.
bool launch_transpose_claim_and_sort(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long columns, long long nnz,
                                     const int* offsetsT, int* cursor, int* work, unsigned long long* keys)
{
    if (nnz <= 0) return true;
    if (!MGCG_HIP(hipMemcpyAsync(cursor, offsetsT, sizeof(int) * (size_t)columns, hipMemcpyDeviceToDevice, s)) || !MGCG_HIP(hipMemsetAsync(work, 0, sizeof(int), s))) return false;
    hipLaunchKernelGGL(transpose_claim_kernel, dim3(transpose_grid(nnz)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, rows, nnz, cursor, keys);
    hipLaunchKernelGGL(transpose_sort_short_kernel, dim3(transpose_grid(columns)), dim3(kBlock), 0, s, offsetsT, columns, keys, work);
    if (nnz > kTransposeShortMax) {
        hipLaunchKernelGGL(transpose_sort_lds_kernel, dim3(kMaxGrid), dim3(kBlock), 0, s, offsetsT, work, keys);
        if (nnz > kTransposeLdsMax) hipLaunchKernelGGL(transpose_sort_global_kernel, dim3(kTransposeLongGrid), dim3(kTransposeLongBlock), 0, s, offsetsT, work, keys);
    }
    return MGCG_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- emit
__global__ __launch_bounds__(kBlock) void transpose_emit_kernel(long long nnz, const TransposeKey* __restrict__ keys, const double* __restrict__ elements,
                                                                int* __restrict__ outColumns, int* __restrict__ outSource, double* __restrict__ outElements)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += stride) {
        const TransposeKey key = keys[q];
        const int k = (int)(key >> 32);
        outColumns[q] = (int)(key & 0xffffffffULL);
        if (outSource != nullptr) outSource[q] = k;
        if (outElements != nullptr) outElements[q] = elements[k];
    }
}
void launch_transpose_emit(hipStream_t s, long long nnz, const unsigned long long* keys, const double* elements, int* outColumns, int* outSource, double* outElements)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(transpose_emit_kernel, dim3(transpose_grid(nnz)), dim3(kBlock), 0, s, nnz, keys, elements, outColumns, outSource, outElements);
}

// ---------------------------------------------------------------- the merged matrix [A | A^T] (square, n rows)
// mergedOffsets[i] = rowOffsets[i] + offsetsT[i]; row i = A's row i in stored order (entry k lands at k + offsetsT[i]), then A^T's row i
// (entry q lands at rowOffsets[i + 1] + q); mergedSource = the stored position in A that the entry's value comes from
__global__ __launch_bounds__(kBlock) void transpose_merged_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                                  const int* __restrict__ offsetsT, const TransposeKey* __restrict__ keys, long long n, long long nnz,
                                                                  int* __restrict__ mergedOffsets, int* __restrict__ mergedColumns, int* __restrict__ mergedSource)
{
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long i = first; i <= n; i += stride) mergedOffsets[i] = rowOffsets[i] + offsetsT[i];
    for (long long k = first; k < nnz; k += stride) {
        const long long p = k + offsetsT[transpose_row_of(rowOffsets, n, k)];
        mergedColumns[p] = columnIndeces[k];
        mergedSource[p] = (int)k;
    }
    for (long long q = first; q < nnz; q += stride) {
        const long long p = q + rowOffsets[transpose_row_of(offsetsT, n, q) + 1];
        const TransposeKey key = keys[q];
        mergedColumns[p] = (int)(key & 0xffffffffULL);
        mergedSource[p] = (int)(key >> 32);
    }
}
void launch_transpose_merged(hipStream_t s, const int* rowOffsets, const int* columnIndeces, const int* offsetsT, const unsigned long long* keys, long long n, long long nnz,
                             int* mergedOffsets, int* mergedColumns, int* mergedSource)
{
    hipLaunchKernelGGL(transpose_merged_kernel, dim3(transpose_grid(nnz > n ? nnz : n + 1)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, offsetsT, keys, n, nnz,
                       mergedOffsets, mergedColumns, mergedSource);
}

void preload_kernels_transpose() { preload_code_object(reinterpret_cast<const void*>(&transpose_emit_kernel)); }

} // namespace mgcg
