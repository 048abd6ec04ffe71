// Multicolour ILU(0) (gfx950; MgSetupIlu0): the row checks, the permuted copy B = P (A + shift diag(A)) P^T with every row sorted by new
// column, the factorisation in place colour by colour, and the two triangular passes of z = U^-1 L^-1 r.  The contract is written out in
// include/MgcgGpu.h; tests/test_ilu_host.py states it in numpy and the kernels here must EQUAL it: every product is rounded before its
// subtraction (the library is built with -ffp-contract=off), a row's sum is a serial sum in stored order from +0.0.
// New row i is the i-th row of the list sorted by (colour, old row): the rows of a colour are one contiguous range, and they store no entry
// of each other (gs_check_kernel has verified it on A), so a launch over one colour reads nothing that another lane group of it writes.
#include "common.hpp"

namespace mgcg {

static inline int ilu_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}
template <int G> static inline int ilu_group_grid(long long rows)
{
    long long b = (rows + kBlock / G - 1) / (kBlock / G);
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- set-up: the rows of A as given
// flags[0 .. 2] (pre-set to INT_MAX) = the smallest row that stores a column outside [0, n), that is empty, that stores no diagonal
__global__ __launch_bounds__(kBlock) void ilu_check_rows_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long n, int* flags)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int k0 = rowOffsets[i], k1 = rowOffsets[i + 1];
        if (k1 == k0) { atomicMin(flags + 1, (int)i); continue; }
        bool outside = false, diagonal = false;
        for (int k = k0; k < k1; ++k) {
            const int j = columnIndeces[k];
            outside |= j < 0 || j >= n;
            diagonal |= j == i;
        }
        if (outside) atomicMin(flags, (int)i);
        if (!diagonal) atomicMin(flags + 2, (int)i);
    }
}
void launch_ilu_check_rows(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, int* flags3)
{
    hipLaunchKernelGGL(ilu_check_rows_kernel, dim3(ilu_grid(n)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, n, flags3);
}

// lengths[i] = the length of old row rowOf[i], lengths[n] = 0: exclusive_scan makes B's offsets of them
__global__ __launch_bounds__(kBlock) void ilu_lengths_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ rowOf, long long n, int* __restrict__ lengths)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
        int len = 0;
        if (i < n) { const int old = rowOf[i]; len = rowOffsets[old + 1] - rowOffsets[old]; }
        lengths[i] = len;
    }
}
void launch_ilu_lengths(hipStream_t s, const int* rowOffsets, const int* rowOf, long long n, int* lengths)
{
    hipLaunchKernelGGL(ilu_lengths_kernel, dim3(ilu_grid(n + 1)), dim3(kBlock), 0, s, rowOffsets, rowOf, n, lengths);
}

// B's rows: G adjacent lanes per new row.  A lane takes the entries e = sub, sub + G, ... of the old row, renumbers the column and finds
// the entry's place by counting the row's entries that sort before it, by (new column, stored position): a rank sort, m^2 / G column
// gathers per lane for a row of m entries, all of them hits of the row's own lines.  An entry that meets its own new column elsewhere
// in the row is a duplicate: *dupRow (pre-set to INT_MAX) = the smallest such OLD row.  The diagonal entry takes a + shift * a (the product
// rounded first) and its place goes to diagPos.
template <int G>
__global__ __launch_bounds__(kBlock) void ilu_build_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                           const int* __restrict__ rowOf, const int* __restrict__ newOf, long long n, double shift,
                                                           const int* __restrict__ offsetsB, double* __restrict__ valuesB, int* __restrict__ columnsB,
                                                           int* __restrict__ diagPos, int* dupRow)
{
    constexpr int kRowsPerBlock = kBlock / G;
    const int sub = threadIdx.x % G;
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    for (long long i = (long long)blockIdx.x * kRowsPerBlock + threadIdx.x / G; i < n; i += stride) {
        const int old = rowOf[i], k0 = rowOffsets[old], m = rowOffsets[old + 1] - k0, d0 = offsetsB[i];
        for (int e = sub; e < m; e += G) {
            const int c = newOf[columnIndeces[k0 + e]];
            int rank = 0;
            bool twice = false;
            for (int f = 0; f < m; ++f) {
                const int cf = newOf[columnIndeces[k0 + f]];
                if (cf < c || (cf == c && f < e)) ++rank;
                twice |= cf == c && f != e;
            }
            if (twice) atomicMin(dupRow, old);
            double v = elements[k0 + e];
            if (c == i) {
                const double scaled = shift * v;
                v = v + scaled;
                diagPos[i] = d0 + rank;
            }
            columnsB[d0 + rank] = c;
            valuesB[d0 + rank] = v;
        }
    }
}
void launch_ilu_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, const int* rowOf, const int* newOf, long long n,
                      double shift, const int* offsetsB, double* valuesB, int* columnsB, int* diagPos, int* dupRow, int lanes)
{
#define MGCG_ILU_BUILD(G) hipLaunchKernelGGL(ilu_build_kernel<G>, dim3(ilu_group_grid<G>(n)), dim3(kBlock), 0, s, elements, rowOffsets, columnIndeces, rowOf, newOf, n, shift, \
                                             offsetsB, valuesB, columnsB, diagPos, dupRow)
    if (lanes == 4) MGCG_ILU_BUILD(4); else if (lanes == 8) MGCG_ILU_BUILD(8); else MGCG_ILU_BUILD(16);
#undef MGCG_ILU_BUILD
}

// ---------------------------------------------------------------- set-up: the factor
// One colour: new rows [row0, row0 + count), G adjacent lanes per row.  The entry at place t of a row belongs to lane t % G of its group,
// and only that lane ever reads or writes its value: program order is all the kernel needs within a row.  The eliminations run in stored
// order, e = 0, 1, ... left of the diagonal: the owner of entry e forms l = b_ik * pinv_k, stores it and hands it to the group by a shuffle;
// every lane then takes its own entries right of e, looks their column up in row k's part right of ITS diagonal (binary search: the rows
// are sorted) and subtracts the rounded product l * b_kj where it is stored.  Row k is of an earlier colour: finished by an earlier launch.
// So b_ij meets its k in ascending order, as in the serial IKJ loop, whatever G is.  Both loop bounds are wavefront-uniform where a shuffle
// stands.  The owner of the diagonal forms pinv_i = 1.0 / b_ii; a pivot that is zero or not finite raises *badRow (pre-set to INT_MAX,
// integer atomicMin) with the OLD row.
template <int G>
__global__ __launch_bounds__(kBlock) void ilu_factor_kernel(int row0, int count, const int* __restrict__ offsetsB, const int* __restrict__ columnsB,
                                                            const int* __restrict__ diagPos, double* valuesB, double* pinv, const int* __restrict__ rowOf, int* badRow)
{
    constexpr int kRowsPerWave = 64 / G, kRowsPerBlock = kBlock / G;
    const int lane = threadIdx.x & 63, sub = lane % G, first = lane - sub;
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    for (long long q0 = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6) * kRowsPerWave; q0 < count; q0 += stride) {
        const long long q = q0 + lane / G;
        const bool live = q < count;
        int i = 0, k0 = 0, m = 0, nl = 0;
        if (live) { i = row0 + (int)q; k0 = offsetsB[i]; m = offsetsB[i + 1] - k0; nl = diagPos[i] - k0; }
        for (int e = 0; __any(e < nl); ++e) {
            const int owner = e % G;
            const bool mine = e < nl;
            int k = 0;
            double lv = 0.0;
            if (mine) k = columnsB[k0 + e];
            if (mine && sub == owner) { lv = valuesB[k0 + e] * pinv[k]; valuesB[k0 + e] = lv; }
            const double l = __shfl(lv, first + owner, 64);
            if (mine) {
                const int u0 = diagPos[k] + 1, u1 = offsetsB[k + 1];
                int t = e + 1;
                t += ((sub - t) % G + G) % G;                          // the lane's first own entry right of e
                for (; t < m; t += G) {
                    const int j = columnsB[k0 + t];
                    int lo = u0, hi = u1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (columnsB[mid] < j) lo = mid + 1; else hi = mid;
                    }
                    if (lo < u1 && columnsB[lo] == j) {
                        const double p = l * valuesB[lo];
                        valuesB[k0 + t] = valuesB[k0 + t] - p;
                    }
                }
            }
        }
        if (live && sub == nl % G) {
            const double pivot = valuesB[k0 + nl];
            if (pivot == 0.0 || !(fabs(pivot) <= 1.7976931348623157e308)) atomicMin(badRow, rowOf[i]);
            pinv[i] = 1.0 / pivot;
        }
    }
}
void launch_ilu_factor(hipStream_t s, int row0, int count, const int* offsetsB, const int* columnsB, const int* diagPos, double* valuesB, double* pinv,
                       const int* rowOf, int* badRow, int lanes)
{
    if (count <= 0) return;
#define MGCG_ILU_FACTOR(G) hipLaunchKernelGGL(ilu_factor_kernel<G>, dim3(ilu_group_grid<G>(count)), dim3(kBlock), 0, s, row0, count, offsetsB, columnsB, diagPos, valuesB, pinv, rowOf, badRow)
    if (lanes == 4) MGCG_ILU_FACTOR(4); else if (lanes == 8) MGCG_ILU_FACTOR(8); else MGCG_ILU_FACTOR(16);
#undef MGCG_ILU_FACTOR
}

// partials[2 b], partials[2 b + 1] = the smallest and the largest pivot b_ii of the rows block b visits (every block visits one at least:
// the grid has no more blocks than n / kBlock rounded up)
__global__ __launch_bounds__(kBlock) void ilu_pivot_range_kernel(const double* __restrict__ valuesB, const int* __restrict__ diagPos, long long n, double* __restrict__ partials)
{
    __shared__ double lo[kBlock], hi[kBlock];
    const long long stride = (long long)gridDim.x * kBlock;
    double a = __builtin_inf(), b = -__builtin_inf();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double pivot = valuesB[diagPos[i]];
        a = fmin(a, pivot); b = fmax(b, pivot);
    }
    lo[threadIdx.x] = a; hi[threadIdx.x] = b;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + w]); hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + w]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = lo[0]; partials[2 * blockIdx.x + 1] = hi[0]; }
}
int launch_ilu_pivot_range(hipStream_t s, const double* valuesB, const int* diagPos, long long n, double* partials)
{
    const int grid = ilu_grid(n);
    hipLaunchKernelGGL(ilu_pivot_range_kernel, dim3(grid), dim3(kBlock), 0, s, valuesB, diagPos, n, partials);
    return grid;
}

// ---------------------------------------------------------------- the application
// One colour of a pass: new rows [row0, row0 + count), a contiguous stretch of the factor; G adjacent lanes per row, and the sum taken in
// stored order by every lane of the group through shuffles, exactly as gs_sweep_kernel<G> takes it (kernels_gs.hip): the serial sum of the
// contract whatever G is, in every mode.  The factor's values and columns are read once per application and not again before the whole
// factor has gone by: non-temporal loads.  y and t are gathered at the columns and written at the rows of the same launch -- never the same
// index, the colour's rows store no entry of each other -- so they carry no __restrict__.
//   forward:   s over the entries left of the diagonal of l_ik * y_k;   y_i = r[rowOf[i]] - s
//   backward:  s over the entries right of it of u_ij * t_j;            t_i = pinv_i * (y_i - s);  z[rowOf[i]] = t_i
template <int G, bool BACKWARD>
__global__ __launch_bounds__(kBlock) void ilu_pass_kernel(int row0, int count, const double* __restrict__ valuesB, const int* __restrict__ offsetsB,
                                                          const int* __restrict__ columnsB, const int* __restrict__ diagPos, const double* __restrict__ pinv,
                                                          const int* __restrict__ rowOf, const double* __restrict__ r, double* y, double* t, double* __restrict__ z,
                                                          const int* done)
{
    if (done != nullptr && *done != 0) return;
    constexpr int kRowsPerWave = 64 / G, kRowsPerBlock = kBlock / G;
    const int lane = threadIdx.x & 63, sub = lane % G, first = lane - sub;
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    const double* x = BACKWARD ? t : y;
    for (long long q0 = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6) * kRowsPerWave; q0 < count; q0 += stride) {
        const long long q = q0 + lane / G;
        const bool live = q < count;
        int i = 0, k0 = 0, m = 0;
        if (live) {
            i = row0 + (int)q;
            const int d = diagPos[i];
            if (BACKWARD) { k0 = d + 1; m = offsetsB[i + 1] - k0; }
            else { k0 = offsetsB[i]; m = d - k0; }
        }
        double sum = 0.0;
        for (int base = 0; __any(base < m); base += G) {
            double p = 0.0;
            if (base + sub < m) {
                const int k = k0 + base + sub;
                p = __builtin_nontemporal_load(valuesB + k) * x[__builtin_nontemporal_load(columnsB + k)];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const double v = __shfl(p, first + u, 64);
                if (base + u < m) sum += v;
            }
        }
        if (live && sub == 0) {
            if (BACKWARD) {
                const double res = y[i] - sum;
                const double ti = pinv[i] * res;
                t[i] = ti;
                z[rowOf[i]] = ti;
            }
            else y[i] = r[rowOf[i]] - sum;
        }
    }
}
void launch_ilu_pass(hipStream_t s, bool backward, int row0, int count, const double* valuesB, const int* offsetsB, const int* columnsB, const int* diagPos,
                     const double* pinv, const int* rowOf, const double* r, double* y, double* t, double* z, int lanes, const int* done)
{
    if (count <= 0) return;
#define MGCG_ILU_PASS(G, B) hipLaunchKernelGGL((ilu_pass_kernel<G, B>), dim3(ilu_group_grid<G>(count)), dim3(kBlock), 0, s, row0, count, valuesB, offsetsB, columnsB, diagPos, \
                                               pinv, rowOf, r, y, t, z, done)
    if (backward) { if (lanes == 4) MGCG_ILU_PASS(4, true); else if (lanes == 8) MGCG_ILU_PASS(8, true); else MGCG_ILU_PASS(16, true); }
    else { if (lanes == 4) MGCG_ILU_PASS(4, false); else if (lanes == 8) MGCG_ILU_PASS(8, false); else MGCG_ILU_PASS(16, false); }
#undef MGCG_ILU_PASS
}

void preload_kernels_ilu() { preload_code_object(reinterpret_cast<const void*>(&ilu_pass_kernel<8, false>)); }

} // namespace mgcg
