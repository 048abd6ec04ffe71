// Multicolour Gauss-Seidel smoothing of the aggregation V-cycle (gfx950; MgSetSmoother(mg, 1)): the colouring round, the colour check and
// the in-place sweep over one colour's row list.  The algorithm is written out in include/MgcgGpu.h; tests/test_gs_host.py states it in
// numpy and the kernels here must EQUAL it: a row's sum is a serial sum in stored order from +0.0 of the rounded products (the library is
// built with -ffp-contract=off), then res = b - s, t = dinv * res, step = omega * t, x = x + step -- the roundings of the Jacobi sweep.
// Rows of one colour hold no stored entry of each other (gs_check_kernel has verified it), so a lane of the sweep reads no value that
// another lane of the same launch writes: the in-place update is race-free and its result does not depend on the schedule.
#include "common.hpp"

namespace mgcg {

static inline int gs_grid(long long n)
{
    long long b = (n + kBlock - 1) / kBlock;
    if (b > kMaxGrid) b = kMaxGrid;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- set-up: the colouring
// the key of a row, 32-bit unsigned arithmetic; rows compare by (key, index)
__device__ __forceinline__ unsigned gs_row_key(unsigned i)
{
    unsigned h = i * 0x9E3779B1u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

// One round.  colourIn[] is the state at the start of the round (-1: uncoloured) and is read only; every row writes its own colourOut[i]:
// no lane depends on another lane of this launch.  An uncoloured row whose (key, index) is larger than that of each of its uncoloured
// neighbours (the columns j != i of its stored entries, whatever their value) takes the smallest colour none of its coloured neighbours
// holds.  flags[0] = 1 if some row is still uncoloured after the round; *badRow (pre-set to INT_MAX) = the smallest row whose coloured
// neighbours hold all 64 colours.
__global__ __launch_bounds__(kBlock) void gs_colour_round_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long n,
                                                                 const int* __restrict__ colourIn, int* __restrict__ colourOut, int* flags, int* badRow)
{
    bool left = false;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int mine = colourIn[i];
        if (mine < 0) {
            const unsigned hi = gs_row_key((unsigned)i);
            unsigned long long held = 0ull;
            bool largest = true;
            for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
                const int j = columnIndeces[k];
                if (j == i || j < 0 || j >= n) continue;
                const int cj = colourIn[j];
                if (cj >= 0) { held |= 1ull << cj; continue; }
                const unsigned hj = gs_row_key((unsigned)j);
                if (hj > hi || (hj == hi && j > i)) { largest = false; break; }
            }
            if (largest) {
                if (held == ~0ull) atomicMin(badRow, (int)i);
                else mine = __ffsll((long long)~held) - 1;
            }
            if (mine < 0) left = true;
        }
        colourOut[i] = mine;
    }
    if (left) flags[0] = 1;
}
void launch_gs_colour_round(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, const int* colourIn, int* colourOut, int* flags, int* badRow)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gs_colour_round_kernel, dim3(gs_grid(n)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, n, colourIn, colourOut, flags, badRow);
}

// *badRow (pre-set to INT_MAX) = the smallest row i that stores an entry (i, j), j != i, with colour[i] == colour[j].  The rounds above give
// two rows that SEE each other different colours; a pair can share one only when j stores i and i does not store j.
__global__ __launch_bounds__(kBlock) void gs_check_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long n,
                                                          const int* __restrict__ colour, int* badRow)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int ci = colour[i];
        for (int k = rowOffsets[i]; k < rowOffsets[i + 1]; ++k) {
            const int j = columnIndeces[k];
            if (j == i) continue;
            if (j < 0 || j >= n || colour[j] == ci) { atomicMin(badRow, (int)i); break; }
        }
    }
}
void launch_gs_check(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, const int* colour, int* badRow)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gs_check_kernel, dim3(gs_grid(n)), dim3(kBlock), 0, s, rowOffsets, columnIndeces, n, colour, badRow);
}

// ---------------------------------------------------------------- the cycle
// x = +0.0 on all rows: where the first sweep of a cycle starts (the sweep then runs its general form: the same bits by construction)
__global__ __launch_bounds__(kBlock) void gs_zero_kernel(long long n, double* __restrict__ x, const int* done)
{
    if (done != nullptr && *done != 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] = 0.0;
}
void launch_gs_zero(hipStream_t s, long long n, double* x, const int* done)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gs_zero_kernel, dim3(gs_grid(n)), dim3(kBlock), 0, s, n, x, done);
}

// One colour of a sweep: G adjacent lanes per row of the list.  The lanes of a group load G consecutive entries of the row at once (one
// coalesced piece of the value and column arrays) and gather x for them in parallel -- the loads are what the pass waits for -- and form the
// rounded products; the SUM is then taken in stored order all the same: every lane of the group adds the G products one after the other,
// fetched from their lanes by shuffles, to a sum that started at +0.0 (a product beyond the row's end is skipped, not added as a zero).
// So the result is the serial sum of the contract whatever G is, in every mode.  (One lane per row, the obvious form for rows this short,
// walks a chain of two dependent loads per entry and ran at an eighth of the byte model's rate: DESIGN section 26.)
// Every lane of a wavefront takes the same trips of both loops (the bounds are wavefront-uniform), so the shuffles find their lanes live.
// b, dinv and x of the row itself are gathered through the list (4 bytes per row).  x is read and written through one pointer: no
// __restrict__ on it; a group writes its x_i after the last product that reads it (the sum depends on all of them).
template <int G>
__global__ __launch_bounds__(kBlock) void gs_sweep_kernel(const int* __restrict__ rows, int count, const double* __restrict__ elements,
                                                          const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                          const double* __restrict__ b, const double* __restrict__ dinv, double omega, double* x, const int* done)
{
    if (done != nullptr && *done != 0) return;
    constexpr int kRowsPerWave = 64 / G, kRowsPerBlock = kBlock / G;
    const int lane = threadIdx.x & 63, sub = lane % G, first = lane - sub;
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    for (long long q0 = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6) * kRowsPerWave; q0 < count; q0 += stride) {
        const long long q = q0 + lane / G;
        const bool live = q < count;
        int i = 0, k0 = 0, m = 0;
        if (live) { i = rows[q]; k0 = rowOffsets[i]; m = rowOffsets[i + 1] - k0; }
        double sum = 0.0;
        for (int base = 0; __any(base < m); base += G) {
            double p = 0.0;
            if (base + sub < m) { const int k = k0 + base + sub; p = elements[k] * x[columnIndeces[k]]; }
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const double v = __shfl(p, first + t, 64);
                if (base + t < m) sum += v;
            }
        }
        if (live && sub == 0) {
            const double res = b[i] - sum;
            const double t = dinv[i] * res;
            const double step = omega * t;
            x[i] = x[i] + step;
        }
    }
}

template <int G>
static void gs_sweep_launch(hipStream_t s, const int* rows, int count, const double* elements, const int* rowOffsets, const int* columnIndeces,
                            const double* b, const double* dinv, double omega, double* x, const int* done)
{
    long long blocks = ((long long)count + kBlock / G - 1) / (kBlock / G);
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    hipLaunchKernelGGL(gs_sweep_kernel<G>, dim3((int)blocks), dim3(kBlock), 0, s, rows, count, elements, rowOffsets, columnIndeces, b, dinv, omega, x, done);
}

// rows[0 .. count): one colour's rows, ascending.  avgRow: the level's entries per row, which picks the lanes per row (4, 8 or 16)
void launch_gs_sweep(hipStream_t s, const int* rows, int count, const double* elements, const int* rowOffsets, const int* columnIndeces,
                     const double* b, const double* dinv, double omega, double* x, double avgRow, const int* done)
{
    if (count <= 0) return;
    if (avgRow <= 4.0) gs_sweep_launch<4>(s, rows, count, elements, rowOffsets, columnIndeces, b, dinv, omega, x, done);
    else if (avgRow <= 10.0) gs_sweep_launch<8>(s, rows, count, elements, rowOffsets, columnIndeces, b, dinv, omega, x, done);
    else gs_sweep_launch<16>(s, rows, count, elements, rowOffsets, columnIndeces, b, dinv, omega, x, done);
}

void preload_kernels_gs() { preload_code_object(reinterpret_cast<const void*>(&gs_sweep_kernel<8>)); }

} // namespace mgcg
