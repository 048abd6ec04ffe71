// Propagation-blocking form for matrices whose gathers have no locality (class 5 of the opt-in analysis, compression mode 3;
// BASELINE config 5: random SPD, 10 M rows, ~31 nonzeros per row spread over the whole column range).
//
// The column-tile form (class 4, kernels_tiled.hip) is bound by the L1 miss path of its gathers.  Here x is
// gathered from LDS instead, and the products travel through memory once:
//   pass 1 (column-tile major): a workgroup holds the x window of one tile of kPbTileWidth columns in LDS (128 KB), streams the tile's
//           entries (8-byte value + 16-bit column offset inside the tile) and stores every rounded product v * x[col] where its entry
//           lies -- one contiguous stream, no destination array;
//   pass 2 (row-block major):   a workgroup owns a block of kPbRows rows, one row per thread.  The block's entries, in their tile-major
//           order (its piece of every tile, one after the other), are taken in ROUNDS of kPbRoundCap entries; for each round the
//           products go to LDS at their position among the round's entries in CSR order, and every row adds its share left to right and
//           carries the sum into the next round.  A row's entries appear in that order in stored order (tiles ascend along a row -- the
//           analysis requires it -- and a row's run inside a tile stays together), so a round may cut a piece anywhere and the additions
//           are still in stored order: bit-identical to the CSR kernels and to the oracle.  The epilogue is applied to the row sum in its
//           register; y is read (beta != 0) and written once per row.
// Layout (all built on the device, pb_build below):
//   entries, tile major, block major inside a tile:  pbVals[k] (8 B), pbCols[k] = column - tile * kPbTileWidth (2 B),
//           pbPos[k] = position of entry k among the entries of its (block, round) in CSR order (2 B), pbProd[k] (8 B, pass 1 output);
//   pbPiece[b * T + t]      first entry of block b inside tile t (row nBlocks: the tile ends);
//   pbPieceOff[b * (T + 1) + t]  where that piece starts in the block's tile-major order (t = T: the block's entry count);
//   pbRoundOff[b]           block b's rounds are numbered pbRoundOff[b] .. pbRoundOff[b + 1] - 1;
//   pbRowBounds             per (block, round) kPbRows + 1 16-bit starts of the rows among the round's entries.
// The 16-bit fields are relative to their round, so a block may hold any number of entries and a piece may be longer than a round (the
// real config-5 matrix has both: blocks of 140 K entries and pieces of 40 K at its end, where the lower triangle piles up).
// Refused at set-up (never clamped in a kernel): rows whose tiles step back, more than kPbMaxTiles tiles, nnz >= 2^31, or more than half
// of the free device memory (about 20 B per entry plus the tables; 24 B per entry while the form is built).
#include "common.hpp"
#include "spmv_epilogue.hpp"

namespace mgcg {

constexpr int kPbThreads = 1024;                 // threads per workgroup of both passes and of the set-up kernels
constexpr int kPbRows = kPbThreads;              // rows per block (one per thread of pass 2)
constexpr int kPbLanes = 64;                     // pass 2: lanes per piece (a wavefront) ...
constexpr int kPbGroups = kPbThreads / kPbLanes; // ... 16 pieces side by side ...
constexpr int kPbUnroll = 10;                    // ... and 10 of those in flight per lane
constexpr int kPbParts = 2;                      // pass 1: workgroups per tile
constexpr int kPbPass1Unroll = 2;                // pass 1: entries per thread in flight
constexpr int kPbChunk = 8;                      // pass 2: consecutive workgroups' blocks per XCD
static_assert(kMaxPartials % (8 * kPbChunk) == 0, "pass 2's grid is a multiple of 8 * kPbChunk");

static_assert(kPbTileWidth == (1 << kPbTileShift), "tile width");
static_assert(kPbRoundCap <= 65535, "positions and row bounds are 16-bit");
// pass 2 LDS: the round, the piece table and the dot reduction must leave room for two workgroups per CU (160 KiB)
static_assert(kPbRoundCap * 8 + kPbMaxTiles * 8 + 4 + 16 * 8 <= 80 * 1024, "two pass-2 workgroups per CU");

static void pb_decline(const char* fmt, ...)
{
    if (tuning().verbose.load(std::memory_order_relaxed) == 0) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fprintf(stderr, "[MgcgGpu] propagation-blocking form (class 5) declined: %s\n", buf);
}

// ---------------------------------------------------------------- set-up kernels
// Block b (one row per thread): entries per tile of the block, written tile major (cells[t * nBlocks + b]); flags[0] rows whose tiles
// step back, flags[1] columns outside [0, columns), flags[2] the largest piece (atomicMax).
__global__ __launch_bounds__(kPbThreads) void pb_count_kernel(const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces, long long rows,
                                                              long long columns, int nTiles, int nBlocks, int* __restrict__ cells, int* __restrict__ flags)
{
    __shared__ int s_cnt[kPbMaxTiles];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    for (int t = tid; t < nTiles; t += kPbThreads) s_cnt[t] = 0;
    __syncthreads();
    const long long row = (long long)b * kPbRows + tid;
    if (row < rows) {
        const int s = rowOffsets[row], e = rowOffsets[row + 1];
        int tile = -1, run = 0, back = 0, outside = 0;
        for (int k = s; k < e; ++k) {
            const int c = columnIndeces[k];
            if (c < 0 || (long long)c >= columns) { outside = 1; continue; }
            const int t = c >> kPbTileShift;
            if (t != tile) {
                if (t < tile) back = 1;
                if (run > 0) atomicAdd(&s_cnt[tile], run);
                tile = t; run = 0;
            }
            ++run;
        }
        if (run > 0) atomicAdd(&s_cnt[tile], run);
        if (back) atomicAdd(&flags[0], 1);
        if (outside) atomicAdd(&flags[1], 1);
    }
    __syncthreads();
    int largest = 0;
    for (int t = tid; t < nTiles; t += kPbThreads) { const int v = s_cnt[t]; cells[(long long)t * nBlocks + b] = v; largest = v > largest ? v : largest; }
    if (largest > 0) atomicMax(&flags[2], largest);
}

// After the exclusive scan of the cells: the block-major piece table (row nBlocks = the tile ends) and the tile starts
__global__ __launch_bounds__(kBlock) void pb_table_kernel(const int* __restrict__ cells, int nTiles, int nBlocks, unsigned* __restrict__ piece, int* __restrict__ tileStart)
{
    const long long n = (long long)(nBlocks + 1) * nTiles;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int b = (int)(i / nTiles), t = (int)(i - (long long)b * nTiles);
        piece[i] = (unsigned)cells[(long long)t * nBlocks + b];      // (b == nBlocks: the first cell of tile t + 1, or the total)
    }
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t <= nTiles; t += stride) tileStart[t] = cells[t * nBlocks];
}

// Rounds per block: the block's entries in their tile-major order (its pieces one after the other) are cut into rounds of kPbRoundCap
// entries, the last one shorter; an empty block has one empty round.  counts[b] = rounds (scanned into pbRoundOff afterwards),
// flags[3] = most rounds of a block.
__global__ __launch_bounds__(kBlock) void pb_rounds_kernel(const int* __restrict__ rowOffsets, long long rows, int nBlocks, int* __restrict__ counts, int* __restrict__ flags)
{
    const int b = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (b >= nBlocks) return;
    const long long r0 = (long long)b * kPbRows, r1 = r0 + kPbRows < rows ? r0 + kPbRows : rows;
    const int n = rowOffsets[r1] - rowOffsets[r0];
    const int nR = n > 0 ? (n + kPbRoundCap - 1) / kPbRoundCap : 1;
    counts[b] = nR;
    atomicMax(&flags[3], nR);
}

// Block-wide inclusive scan of one int per thread (Hillis-Steele in LDS); returns this thread's inclusive prefix
__device__ __forceinline__ int pb_block_scan(int* s_scan, int v)
{
    const int tid = (int)threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int off = 1; off < kPbThreads; off <<= 1) {
        const int add = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int r = s_scan[tid];
    __syncthreads();                                                // (s_scan may be reused at once)
    return r;
}

// Block b (one row per thread).  First every (row, tile) run reserves a contiguous chunk of its piece (the order of the chunks inside a
// piece is the order the rows reach it; a row's entries keep their stored order) and its entries go there with their 16-bit column
// offsets; flat[k] = the entry's index in the block's tile-major order (pieceOff[b * (T + 1) + t] = where piece t starts in that order,
// also written here).  A row's flat indices ascend along the row, so every round holds a contiguous stretch of every row: then the rows'
// starts among each round's entries in CSR order go to rowBounds and every entry's position among them to pos.  flags[5] is raised if
// any piece is not filled exactly.
__global__ __launch_bounds__(kPbThreads) void pb_place_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                              long long rows, int nTiles, const unsigned* __restrict__ piece, unsigned* __restrict__ pieceOff,
                                                              const int* __restrict__ roundOff, int* __restrict__ flat, double* __restrict__ vals, unsigned short* __restrict__ cols,
                                                              unsigned short* __restrict__ pos, unsigned short* __restrict__ rowBounds, int* __restrict__ flags)
{
    __shared__ unsigned s_cur[kPbMaxTiles];
    __shared__ unsigned s_start[kPbMaxTiles];
    __shared__ unsigned s_off[kPbMaxTiles + 1];
    __shared__ int s_scan[kPbThreads];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    {   // piece starts and their offsets in the block's order (nTiles <= kPbThreads: one tile per thread)
        const unsigned st = tid < nTiles ? piece[(long long)b * nTiles + tid] : 0u;
        const int len = tid < nTiles ? (int)(piece[(long long)(b + 1) * nTiles + tid] - st) : 0;
        const int inc = pb_block_scan(s_scan, len);
        if (tid < nTiles) { s_cur[tid] = st; s_start[tid] = st; s_off[tid] = (unsigned)(inc - len); }
        if (tid == kPbThreads - 1) s_off[nTiles] = (unsigned)inc;
    }
    __syncthreads();
    for (int t = tid; t <= nTiles; t += kPbThreads) pieceOff[(long long)b * (nTiles + 1) + t] = s_off[t];
    const long long row = (long long)b * kPbRows + tid;
    int e0 = 0, eEnd = 0;
    if (row < rows) { e0 = rowOffsets[row]; eEnd = rowOffsets[row + 1]; }
    for (int k = e0; k < eEnd;) {
        const int t = columnIndeces[k] >> kPbTileShift;
        int m = k + 1;
        while (m < eEnd && (columnIndeces[m] >> kPbTileShift) == t) ++m;
        const unsigned slot0 = atomicAdd(&s_cur[t], (unsigned)(m - k));
        for (int q = k; q < m; ++q) {
            const unsigned slot = slot0 + (unsigned)(q - k);
            vals[slot] = elements[q];
            cols[slot] = (unsigned short)(columnIndeces[q] - (t << kPbTileShift));
            flat[q] = (int)(s_off[t] + (slot - s_start[t]));
        }
        k = m;
    }
    const int ro = roundOff[b], nR = roundOff[b + 1] - ro;
    int e = e0;
    for (int j = 0; j < nR; ++j) {
        const int q1 = (j + 1) * kPbRoundCap;
        int f = e;
        while (f < eEnd && flat[f] < q1) ++f;
        const int cnt = f - e;
        const int start = pb_block_scan(s_scan, cnt) - cnt;
        unsigned short* bounds = rowBounds + (long long)(ro + j) * (kPbRows + 1);
        bounds[tid] = (unsigned short)start;
        if (tid == kPbThreads - 1) bounds[kPbRows] = (unsigned short)(start + cnt);
        for (int q = e; q < f; ++q) {
            const int t = columnIndeces[q] >> kPbTileShift;
            pos[s_start[t] + ((unsigned)flat[q] - s_off[t])] = (unsigned short)(start + (q - e));
        }
        e = f;
    }
    if (e != eEnd) atomicOr(&flags[5], 1);
    __syncthreads();
    for (int t = tid; t < nTiles; t += kPbThreads)
        if (s_cur[t] != piece[(long long)(b + 1) * nTiles + t]) atomicOr(&flags[5], 1);
}

// ---------------------------------------------------------------- SpMV
// Pass 1: prod[k] = vals[k] * x[column of k] for the entries of one tile, x from LDS.  kPbParts workgroups per tile, the LAST tiles first:
// on config 5 the columns near the end hold the most entries (the lower triangle piles up there), so the long tiles start first and the
// short ones fill in behind them; dealing contiguous chunks of tiles to the XCDs, as the lab did on a uniform matrix, put the long ones
// all on one XCD (1.88 ms per pass against 1.1 in the lab).
__global__ __launch_bounds__(kPbThreads) void pb_pass1_kernel(const double* __restrict__ x, long long xLen, const double* __restrict__ vals,
                                                              const unsigned short* __restrict__ cols, const int* __restrict__ tileStart, int nTiles,
                                                              double* __restrict__ prod, const int* __restrict__ doneFlag)
{
    __shared__ double s_x[kPbTileWidth];
    if (doneFlag != nullptr && *doneFlag != 0) return;
    const int t = nTiles - 1 - (int)blockIdx.x / kPbParts, part = (int)blockIdx.x % kPbParts;   // (grid = nTiles * kPbParts)
    const long long c0 = (long long)t * kPbTileWidth;
    for (int i = (int)threadIdx.x; i < kPbTileWidth; i += kPbThreads) { const long long c = c0 + i; s_x[i] = c < xLen ? x[c] : 0.0; }
    __syncthreads();
    const int kb = tileStart[t], ke = tileStart[t + 1];
    const long long len = (long long)ke - kb;
    const int lo = kb + (int)(len * part / kPbParts), hi = kb + (int)(len * (part + 1) / kPbParts);
    for (int k0 = lo; k0 < hi; k0 += kPbThreads * kPbPass1Unroll) {
        double v[kPbPass1Unroll]; unsigned c[kPbPass1Unroll];
#pragma unroll
        for (int u = 0; u < kPbPass1Unroll; ++u) {
            const int k = k0 + u * kPbThreads + (int)threadIdx.x;
            const int kk = k < hi ? k : lo;                         // (lo < hi here: a valid entry)
            v[u] = __builtin_nontemporal_load(vals + kk);
            c[u] = __builtin_nontemporal_load(cols + kk);
        }
#pragma unroll
        for (int u = 0; u < kPbPass1Unroll; ++u) {
            const int k = k0 + u * kPbThreads + (int)threadIdx.x;
            if (k < hi) prod[k] = v[u] * s_x[c[u]];
        }
    }
}

// Pass 2: blocksPer consecutive blocks per workgroup (so that a dot epilogue writes at most kMaxPartials partial sums, one per
// workgroup), the last (longest) blocks first, and kPbChunk consecutive workgroups' blocks on one XCD (workgroup w runs on XCD w % 8):
// neighbouring blocks' pieces share lines of the product stream in that XCD's L2, and the chunks still spread the long blocks over
// every XCD.  Round j of a block is the stretch [j * kPbRoundCap,
// (j + 1) * kPbRoundCap) of its tile-major order: the tail of one piece, whole pieces, the head of another.
template <int EPI>
__global__ __launch_bounds__(kPbThreads) __attribute__((amdgpu_waves_per_eu(8))) void pb_pass2_kernel(SpmvArgs a, const double* __restrict__ prod, const unsigned short* __restrict__ pos,
                                                              const unsigned* __restrict__ piece, const unsigned* __restrict__ pieceOff, const int* __restrict__ roundOff,
                                                              const unsigned short* __restrict__ rowBounds, int nTiles, int nBlocks, int blocksPer)
{
    __shared__ double s[kPbRoundCap];
    __shared__ unsigned s_start[kPbMaxTiles];
    __shared__ unsigned s_off[kPbMaxTiles + 1];
    __shared__ double s_red[kPbThreads / 64];
    if (a.doneFlag != nullptr && *a.doneFlag != 0) return;
    const int tid = (int)threadIdx.x, grp = tid / kPbLanes, l = tid % kPbLanes;
    const int g = (int)blockIdx.x, slot = g >> 3;
    const int unit = (slot / kPbChunk) * (8 * kPbChunk) + (g & 7) * kPbChunk + slot % kPbChunk;
    double dotacc = 0.0;
    for (int bi = 0; bi < blocksPer; ++bi) {
        const int seq = unit * blocksPer + bi;
        if (seq >= nBlocks) break;                                  // (workgroup-uniform)
        const int b = nBlocks - 1 - seq;
        const long long r0 = (long long)b * kPbRows;
        const bool mine = r0 + tid < (long long)a.rowCount;
        const long long row = r0 + tid;
        for (int t = tid; t <= nTiles; t += kPbThreads) {
            if (t < nTiles) s_start[t] = piece[(long long)b * nTiles + t];
            s_off[t] = pieceOff[(long long)b * (nTiles + 1) + t];
        }
        // the epilogue's operands are requested behind the piece table (the Jacobi forms' three operands after the rounds: registers)
        constexpr bool kLate = EPI == EPI_JACOBI || EPI == EPI_JACOBI_DOT;
        RowsEpi o; o.w = 0.0; o.b = 0.0; o.dinv = 0.0; o.yold = 0.0;
        if (!kLate && mine) o = rows_epi_prefetch<EPI>(a, row);
        const int ro = roundOff[b], nR = roundOff[b + 1] - ro;
        __syncthreads();
        double acc = 0.0;
        for (int j = 0; j < nR; ++j) {
            const unsigned q0 = (unsigned)j * kPbRoundCap, q1 = q0 + kPbRoundCap < s_off[nTiles] ? q0 + kPbRoundCap : s_off[nTiles];
            // tiles [tLo, tHi) reach into the round: tLo = first t with s_off[t + 1] > q0, tHi = first t with s_off[t] >= q1
            int tLo = 0, tHi = 0;
            for (int hi = nTiles; tLo < hi;) { const int mid = (tLo + hi) >> 1; if (s_off[mid + 1] > q0) hi = mid; else tLo = mid + 1; }
            for (int hi = nTiles; tHi < hi;) { const int mid = (tHi + hi) >> 1; if (s_off[mid] >= q1) hi = mid; else tHi = mid + 1; }
            const unsigned short* bounds = rowBounds + (long long)(ro + j) * (kPbRows + 1);
            const int ra = bounds[tid], re = bounds[tid + 1];
            for (int tb = tLo; tb < tHi; tb += kPbGroups * kPbUnroll) {
                double p[kPbUnroll]; int at[kPbUnroll]; bool ok[kPbUnroll];
#pragma unroll
                for (int u = 0; u < kPbUnroll; ++u) {
                    const int t = tb + grp + u * kPbGroups;
                    unsigned first = 0; int len = 0;
                    if (t < tHi) {
                        const unsigned lo = s_off[t] > q0 ? s_off[t] : q0, hi = s_off[t + 1] < q1 ? s_off[t + 1] : q1;
                        first = s_start[t] + (lo - s_off[t]); len = hi > lo ? (int)(hi - lo) : 0;
                    }
                    ok[u] = l < len;
                    const unsigned src = ok[u] ? first + (unsigned)l : 0u;
                    p[u] = prod[src];
                    at[u] = (int)pos[src];
                }
#pragma unroll
                for (int u = 0; u < kPbUnroll; ++u) if (ok[u]) s[at[u]] = p[u];
                for (int u = 0; u < kPbUnroll; ++u) {                // pieces of more than kPbLanes entries in this round
                    const int t = tb + grp + u * kPbGroups;
                    if (t >= tHi) break;
                    const unsigned lo = s_off[t] > q0 ? s_off[t] : q0, hi = s_off[t + 1] < q1 ? s_off[t + 1] : q1;
                    if (hi <= lo + kPbLanes) continue;
                    const unsigned first = s_start[t] + (lo - s_off[t]), len = hi - lo;
                    for (unsigned i = (unsigned)l + kPbLanes; i < len; i += kPbLanes) s[(int)pos[first + i]] = prod[first + i];
                }
            }
            __syncthreads();
            for (int k = ra; k < re; ++k) acc += s[k];              // (rows past the matrix's end have ra == re)
            __syncthreads();
        }
        if (kLate && mine) o = rows_epi_prefetch<EPI>(a, row);
        if (mine) a.y[row] = rows_epilogue_value<EPI>(a, acc, o, dotacc);
    }
    if constexpr (epi_has_dot(EPI)) {
        double v = dotacc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) s_red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int w = 0; w < kPbThreads / 64; ++w) sum += s_red[w];
            a.partials[blockIdx.x] = sum;
        }
    }
}

template <int EPI>
static int launch_pb_epi(hipStream_t s, const SpmvArgs& a, const DcsrView& m)
{
    const long long xLen = a.columnCount > 0 && (long long)a.columnCount < m.pbColumns ? (long long)a.columnCount : m.pbColumns;
    hipLaunchKernelGGL(pb_pass1_kernel, dim3((unsigned)(m.pbTiles * kPbParts)), dim3(kPbThreads), 0, s, a.x, xLen, m.pbVals, m.pbCols, m.pbTileStart, m.pbTiles,
                       m.pbProd, a.doneFlag);
    const int blocksPer = (m.pbBlocks + kMaxPartials - 1) / kMaxPartials;
    const int units = (m.pbBlocks + blocksPer - 1) / blocksPer;
    const int grid = (units + 8 * kPbChunk - 1) / (8 * kPbChunk) * (8 * kPbChunk);   // <= kMaxPartials (a multiple of 8 * kPbChunk)
    hipLaunchKernelGGL((pb_pass2_kernel<EPI>), dim3((unsigned)grid), dim3(kPbThreads), 0, s, a, m.pbProd, m.pbPos, m.pbPiece, m.pbPieceOff, m.pbRoundOff,
                       m.pbRowBounds, m.pbTiles, m.pbBlocks, blocksPer);
    return grid;
}

int launch_spmv_pb(hipStream_t s, int epilogue, const SpmvArgs& a, const DcsrView& m)
{
    if (a.rowCount <= 0) return 0;
    switch (epilogue) {
    case EPI_AXPBY:        return a.beta != 0.0 ? launch_pb_epi<EPI_AXPBY_BETA>(s, a, m) : launch_pb_epi<EPI_AXPBY>(s, a, m);
    case EPI_AXPBY_BETA:   return launch_pb_epi<EPI_AXPBY_BETA>(s, a, m);
    case EPI_DOT:          return launch_pb_epi<EPI_DOT>(s, a, m);
    case EPI_RESIDUAL:     return launch_pb_epi<EPI_RESIDUAL>(s, a, m);
    case EPI_RESIDUAL_DOT: return launch_pb_epi<EPI_RESIDUAL_DOT>(s, a, m);
    case EPI_JACOBI:       return launch_pb_epi<EPI_JACOBI>(s, a, m);
    case EPI_JACOBI_DOT:   return launch_pb_epi<EPI_JACOBI_DOT>(s, a, m);
    }
    set_error("propagation-blocking SpMV: epilogue %d is not implemented (the Chebyshev step multiplies through the CSR kernels)", epilogue);   // never a silent no-op
    return 0;
}

// ---------------------------------------------------------------- build
// On success out->pbVals != nullptr says whether the form exists.  meanDistance: the sampled mean |col - row| (spmv_period);
// columns: length of x.  Leaves the other fields of *out alone.  false only on a device error.
bool pb_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
              long long rows, long long nnz, long long columns, long long meanDistance, DcsrMatrix* out)
{
    if (rows <= 0 || nnz <= 0) { pb_decline("empty matrix"); return true; }
    if (nnz >= 0x7fffffffLL) { pb_decline("%lld nonzeros (the form indexes them with 32 bits)", nnz); return true; }
    if (meanDistance < kPbTileWidth) { pb_decline("sampled mean distance from the diagonal %lld < one tile (%d columns): the gathers have locality", meanDistance, kPbTileWidth); return true; }
    const long long nTilesL = (columns + kPbTileWidth - 1) / kPbTileWidth;
    if (nTilesL < 2) { pb_decline("x spans %lld tile(s), fewer than 2", nTilesL); return true; }
    if (nTilesL > kPbMaxTiles) { pb_decline("%lld tiles, more than the %d pass 2's table holds", nTilesL, kPbMaxTiles); return true; }
    const int nTiles = (int)nTilesL;
    const long long nBlocksL = (rows + kPbRows - 1) / kPbRows;
    const long long cells = nBlocksL * nTiles;
    if (cells + nBlocksL + 1 >= 0x7fffffffLL) { pb_decline("%lld (block, tile) cells", cells); return true; }
    const int nBlocks = (int)nBlocksL;
    const double rounds = (double)nBlocks + (double)nnz / kPbRoundCap;
    {   // entries 10 B + products 8 B + positions 2 B per nonzero, and 4 B per nonzero while the form is built; cells, piece table and
        // piece offsets 12 B per (block, tile); row bounds 2 KB per (block, round)
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); pb_decline("hipMemGetInfo failed"); return true; }
        const double need = 24.0 * (double)nnz + 12.0 * (double)(cells + nTiles + nBlocks + 1) + 2.0 * (kPbRows + 1) * rounds;
        if (need > 0.5 * (double)freeB) { pb_decline("needs %.2f GB, more than half of the %.2f GB free", need / 1e9, (double)freeB / 1e9); return true; }
    }
    int* cellsD = nullptr; int* flags = nullptr; unsigned* piece = nullptr; unsigned* pieceOff = nullptr; int* tileStart = nullptr; int* roundOff = nullptr;
    unsigned short* rowBounds = nullptr; int* flat = nullptr;
    double* vals = nullptr; unsigned short* cols = nullptr; unsigned short* pos = nullptr; double* prod = nullptr;
    auto fail = [&](bool hard) {
        (void)hipStreamSynchronize(s);
        for (void* p : { (void*)cellsD, (void*)flags, (void*)piece, (void*)pieceOff, (void*)tileStart, (void*)roundOff, (void*)rowBounds, (void*)flat, (void*)vals, (void*)cols,
                         (void*)pos, (void*)prod })
            if (p) (void)hipFree(p);
        if (!hard) (void)hipGetLastError();
        return !hard;
    };
    bool ok = MGCG_HIP(hipMalloc((void**)&cellsD, sizeof(int) * (size_t)(cells + 1))) && MGCG_HIP(hipMalloc((void**)&flags, 8 * sizeof(int))) &&
              MGCG_HIP(hipMemsetAsync(cellsD + cells, 0, sizeof(int), s)) && MGCG_HIP(hipMemsetAsync(flags, 0, 8 * sizeof(int), s));
    if (!ok) return fail(true);
    // 1. entries per (block, tile); rows whose tiles step back, columns outside x
    hipLaunchKernelGGL(pb_count_kernel, dim3((unsigned)nBlocks), dim3(kPbThreads), 0, s, rowOffsets, columnIndeces, rows, columns, nTiles, nBlocks, cellsD, flags);
    int hf[8] = {};
    ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (!ok) return fail(true);
    if (hf[0] != 0) { pb_decline("%d row(s) step back to an earlier column tile", hf[0]); return fail(false); }
    if (hf[1] != 0) { pb_decline("%d row(s) hold columns outside [0, %lld)", hf[1], columns); return fail(false); }
    // 2. piece table and tile starts
    if (!exclusive_scan(s, cellsD, cells + 1)) return fail(true);
    ok = MGCG_HIP(hipMalloc((void**)&piece, sizeof(unsigned) * (size_t)(cells + nTiles))) && MGCG_HIP(hipMalloc((void**)&tileStart, sizeof(int) * (size_t)(nTiles + 1)));
    if (!ok) return fail(true);
    {
        long long g = (cells + nTiles + kBlock - 1) / kBlock;
        if (g > kMaxGrid) g = kMaxGrid;
        hipLaunchKernelGGL(pb_table_kernel, dim3((unsigned)g), dim3(kBlock), 0, s, cellsD, nTiles, nBlocks, piece, tileStart);
    }
    int total = 0;
    ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&total, cellsD + cells, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (!ok) return fail(true);
    if ((long long)total != nnz) { set_error("propagation-blocking analysis: %d of %lld nonzeros counted", total, nnz); return fail(true); }
    (void)hipFree(cellsD); cellsD = nullptr;
    // 3. rounds per block
    ok = MGCG_HIP(hipMalloc((void**)&roundOff, sizeof(int) * (size_t)(nBlocks + 1))) && MGCG_HIP(hipMemsetAsync(roundOff + nBlocks, 0, sizeof(int), s));
    if (!ok) return fail(true);
    hipLaunchKernelGGL(pb_rounds_kernel, dim3((unsigned)((nBlocks + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, rowOffsets, rows, nBlocks, roundOff, flags);
    if (!MGCG_HIP(hipGetLastError()) || !exclusive_scan(s, roundOff, (long long)nBlocks + 1)) return fail(true);
    int roundsTotal = 0;
    ok = MGCG_HIP(hipMemcpyAsync(&roundsTotal, roundOff + nBlocks, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (!ok) return fail(true);
    // 4. + 5. the entries in tile-major order with their positions in their rounds, the piece offsets and the rows' bounds per round
    ok = MGCG_HIP(hipMalloc((void**)&rowBounds, sizeof(unsigned short) * (size_t)roundsTotal * (kPbRows + 1))) &&
         MGCG_HIP(hipMalloc((void**)&pieceOff, sizeof(unsigned) * (size_t)nBlocks * (nTiles + 1))) && MGCG_HIP(hipMalloc((void**)&flat, sizeof(int) * (size_t)nnz)) &&
         MGCG_HIP(hipMalloc((void**)&vals, sizeof(double) * (size_t)nnz)) && MGCG_HIP(hipMalloc((void**)&cols, sizeof(unsigned short) * (size_t)nnz)) &&
         MGCG_HIP(hipMalloc((void**)&pos, sizeof(unsigned short) * (size_t)nnz)) && MGCG_HIP(hipMalloc((void**)&prod, sizeof(double) * (size_t)nnz));
    if (!ok) return fail(true);
    hipLaunchKernelGGL(pb_place_kernel, dim3((unsigned)nBlocks), dim3(kPbThreads), 0, s, elements, rowOffsets, columnIndeces, rows, nTiles, piece, pieceOff, roundOff, flat,
                       vals, cols, pos, rowBounds, flags);
    ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (!ok) return fail(true);
    if (hf[5] != 0) { set_error("propagation-blocking analysis: the entries do not fill their pieces"); return fail(true); }
    (void)hipFree(flags); (void)hipFree(flat);
    out->pbVals = vals; out->pbCols = cols; out->pbPos = pos; out->pbProd = prod; out->pbPiece = piece; out->pbPieceOff = pieceOff; out->pbTileStart = tileStart;
    out->pbRoundOff = roundOff; out->pbRowBounds = rowBounds;
    out->pbTiles = nTiles; out->pbBlocks = nBlocks; out->pbMaxRounds = hf[3]; out->pbColumns = columns;
    return true;
}

void preload_kernels_pb() { preload_code_object(reinterpret_cast<const void*>(&pb_pass1_kernel)); }

} // namespace mgcg
