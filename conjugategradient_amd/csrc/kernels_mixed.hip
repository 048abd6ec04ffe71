// Mixed-precision CG for gfx950 (SolveMixed, MgcgMixedSetup, CsrMVFloat): an fp32 CG recurrence corrected by fp64 reliable updates
// (Sleijpen / van der Vorst; the form QUDA uses).  The loop is HBM-bound, so what an iteration costs is its bytes: with 7 entries per row
// the fp32 product moves 8*7 + 4 + 8 = 68 bytes per row against 104 and the two vector passes 12 + 20 against 64 -- 100 against 168.
//
// The loop (include/MgcgGpu.h has the rounding contract; tests/test_mixed_host.py the same loop in numpy).  x, r and b are fp64; xs (the
// partial solution since the last update), r32, p32 and Ap32 are fp32 and live on the handle's workspace.
//   start        r = b - A x in fp64 ; rr0 = rr = maxrr = r.r ; r32 = (float)r ; p32 = r32 ; xs = 0
//   iteration    Ap32 = A32 p32 ; pAp = sum (double)p_i (double)Ap_i ; alpha = rr / pAp ; xs += alpha32 p32 ; r32 -= alpha32 Ap32 ;
//                rn = sum (double)r_i^2 ; maxrr = max(maxrr, rn) ; want |= rn < 0.01 maxrr, or the stop rule would fire on rn
//   update slot  (iterations with it % 4 == 3, when want is up)  x += (double)xs ; xs = 0 ; r = b - A x with the fp64 matrix ; rn = r.r ;
//                r32 = (float)r ; maxrr = rn ; the stop decision, here and only here, on the true rn
//   end          beta = rn / rr ; p32 = r32 + beta32 p32 ; rr = rn          (p is kept across an update: the recurrence is not restarted)
//
// Launches.  A normal iteration is three: the fp32 product with the partial sums of p.Ap as its epilogue, mixed_update_r_kernel (alpha, the
// r pass, the partial sums of rn, the frozen copies of the scalars) and mixed_update_xp_kernel, which finalises the iteration in every
// workgroup -- the same fixed-order sum of the partial sums everywhere, the first workgroup alone publishing -- and then runs the xs / p32
// pass.  Behind every fourth iteration the host enqueues the three launches of an update without asking the device: mixed_fold_x_kernel,
// the loop's own fp64 residual product (SpmvArgs::doneFlag on the gate) and mixed_restart_kernel.  All three return at their first
// instruction unless the x/p pass of that iteration opened the gate (MixedScalars::gate == 0); every r pass closes it again, also once
// the loop has stopped.  In an update iteration the x/p pass leaves p32 and the publishing to the restart pass, which has the true rn.
//
// Sums.  Per lane in fp64 in index order, then the fixed tree of vec_passes.hpp, one partial per workgroup, no atomics: the same bits on
// every run.  Under dot_order = 1 both dots of the fp32 loop are serial left-to-right sums of the exact fp64 products
// (mixed_dot_serial_kernel), the update's r.r is SolveEx's serial sum, and the long-row form of the product adds a row in stored order.
#include "vec_passes.hpp"

namespace mgcg {

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr double kFloatMax = 3.4028234663852886e38;   // FLT_MAX: a residual with sqrt(r.r) below it converts to finite floats

bool Workspace::ensure_mixed(long long n)
{
    if (!mixedScalars) {
        if (!MGCG_HIP(hipMalloc((void**)&mixedScalars, sizeof(MixedScalars)))) return false;
        if (!MGCG_HIP(hipMemset(mixedScalars, 0, sizeof(MixedScalars)))) { (void)hipFree((void*)mixedScalars); mixedScalars = nullptr; return false; }
    }
    const long long stride = (n + 3) & ~3LL;
    if (mixedVecs && mixedStride >= stride) return true;
    if (stream) (void)hipStreamSynchronize(stream);                    // nothing enqueued may still use the vectors that go
    if (mixedVecs) (void)hipFree(mixedVecs);
    mixedVecs = nullptr; mixedStride = 0;
    if (!MGCG_HIP(hipMalloc((void**)&mixedVecs, sizeof(float) * 4 * (size_t)stride))) return false;
    mixedStride = stride;
    return true;
}

__device__ __forceinline__ long long clamp_offset(long long k, long long nnz) { return k < 0 ? 0 : (k > nnz ? nnz : k); }

// ------------------------------------------------------------------ set-up: e32 = (float)elements
// One lane per entry.  flags (pre-set to {0, 0, INT_MAX}): [0] some value was rounded, [1] some value is not finite as a float, [2] the
// first row that holds one (order-free atomicMin; the row is looked up for this report only: the last row whose offset is <= k).
__global__ __launch_bounds__(kBlock) void mixed_convert_kernel(const double* __restrict__ elements, const int* __restrict__ rowOffsets, long long nnz, long long rows,
                                                               float* __restrict__ e32, int* flags)
{
    grid_stride<false>(nnz, [&](long long) {}, [&](long long k) {
        const double a = elements[k];
        const float f = (float)a;
        e32[k] = f;
        if (!((double)f == a)) flags[0] = 1;                           // (a NaN counts as rounded, and as not finite below)
        if (!(fabs((double)f) <= kFloatMax)) {
            long long lo = 0, hi = rows;                               // first row whose end lies beyond k
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)rowOffsets[mid + 1] > k) hi = mid; else lo = mid + 1; }
            if (lo >= rows) lo = rows > 0 ? rows - 1 : 0;              // (an entry behind the last row's end)
            flags[1] = 1; atomicMin(&flags[2], (int)lo);
        }
    });
}
void launch_mixed_convert(hipStream_t s, const double* elements, const int* rowOffsets, long long nnz, long long rows, float* e32, int* flags)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(mixed_convert_kernel, dim3(grid_for(nnz, 1)), dim3(kBlock), 0, s, elements, rowOffsets, nnz, rows, e32, flags);
}

// ------------------------------------------------------------------ the fp32 product
// Lane = row (mean row length up to 20).  A workgroup takes tiles of 256 rows; the tile's span of values and columns is staged in LDS
// with coalesced 4-byte loads, 2048 entries (16 KB) at a time, and every lane then walks its own row through the staged chunk: the
// row-tile idea of kernels_rowtile.hip with 4-byte values and 4-byte gathers.  A row adds its rounded products in stored order from
// +0.0f, so the form is bit-exact in every mode.  The chunk count is the same in every lane of the workgroup, so the barriers are legal.
constexpr int kF32Chunk = 2048;
template <bool DOT>
__global__ __launch_bounds__(kBlock) void spmv_float_rows_kernel(const float* __restrict__ e32, const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                                 const float* __restrict__ x, float* __restrict__ y, long long nnz, long long rows,
                                                                 double* __restrict__ partials, const int* done)
{
    __shared__ float s_val[kF32Chunk];
    __shared__ int s_col[kF32Chunk];
    __shared__ double s_red[4];
    if (done != nullptr && *done != 0) return;
    const long long tiles = (rows + kBlock - 1) / kBlock;
    double dacc = 0.0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long row0 = t * kBlock, row = row0 + threadIdx.x;
        const long long rowTop = row0 + kBlock < rows ? row0 + kBlock : rows;
        const long long k0 = clamp_offset(rowOffsets[row0], nnz), k1 = clamp_offset(rowOffsets[rowTop], nnz);
        long long a = 0, b = 0;
        if (row < rows) { a = clamp_offset(rowOffsets[row], nnz); b = clamp_offset(rowOffsets[row + 1], nnz); }
        float acc = 0.0f;
        for (long long base = k0; base < k1; base += kF32Chunk) {
            const long long top = base + kF32Chunk < k1 ? base + kF32Chunk : k1;
            __syncthreads();                                           // the chunk before this one has been read by every lane
            for (long long k = base + threadIdx.x; k < top; k += kBlock) { s_val[k - base] = e32[k]; s_col[k - base] = columnIndeces[k]; }
            __syncthreads();
            const long long lo = a > base ? a : base, hi = b < top ? b : top;
            for (long long k = lo; k < hi; ++k) { const float u = s_val[k - base] * x[s_col[k - base]]; acc = acc + u; }
        }
        if (row < rows) {
            y[row] = acc;
            if constexpr (DOT) { const double q = (double)x[row] * (double)acc; dacc += q; }
        }
    }
    if constexpr (DOT) {
        const double t = block_sum(dacc, s_red);
        if (threadIdx.x == 0) partials[blockIdx.x] = t;
    }
}

// L lanes per row (long rows: the driver matrices have 159 entries per row).  Lane l adds the products of entries l, l + L, ... in
// float and the lanes' sums meet in a shuffle tree; SERIAL (dot_order = 1): the row's first lane adds every product in stored order.
template <int L, bool DOT, bool SERIAL>
__global__ __launch_bounds__(kBlock) void spmv_float_vector_kernel(const float* __restrict__ e32, const int* __restrict__ rowOffsets, const int* __restrict__ columnIndeces,
                                                                   const float* __restrict__ x, float* __restrict__ y, long long nnz, long long rows,
                                                                   double* __restrict__ partials, const int* done)
{
    __shared__ double s_red[4];
    if (done != nullptr && *done != 0) return;
    constexpr int kRows = kBlock / L;
    const int lane = threadIdx.x % L, sub = threadIdx.x / L;
    const long long groups = (rows + kRows - 1) / kRows;
    double dacc = 0.0;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long row = g * kRows + sub;
        float acc = 0.0f;
        if (row < rows) {
            const long long a = clamp_offset(rowOffsets[row], nnz), b = clamp_offset(rowOffsets[row + 1], nnz);
            if constexpr (SERIAL) {
                if (lane == 0) for (long long k = a; k < b; ++k) { const float u = e32[k] * x[columnIndeces[k]]; acc = acc + u; }
            } else {
                for (long long k = a + lane; k < b; k += L) { const float u = e32[k] * x[columnIndeces[k]]; acc = acc + u; }
            }
        }
        if constexpr (!SERIAL) {
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, L);
        }
        if (row < rows && lane == 0) {
            y[row] = acc;
            if constexpr (DOT) { const double q = (double)x[row] * (double)acc; dacc += q; }
        }
    }
    if constexpr (DOT) {
        const double t = block_sum(dacc, s_red);
        if (threadIdx.x == 0) partials[blockIdx.x] = t;
    }
}

template <int L>
static int launch_spmv_float_vector(hipStream_t s, const float* e32, const int* rowOffsets, const int* columnIndeces, const float* x, float* y, long long nnz, long long rows,
                                    double* partials, const int* done)
{
    const long long groups = (rows + kBlock / L - 1) / (kBlock / L);
    const int grid = (int)(groups < kMaxGrid ? groups : kMaxGrid);
    with_flags([&](auto DOT, auto SERIAL) {
        hipLaunchKernelGGL((spmv_float_vector_kernel<L, DOT.value, SERIAL.value>), dim3(grid), dim3(kBlock), 0, s, e32, rowOffsets, columnIndeces, x, y, nnz, rows, partials, done);
    }, partials != nullptr, dot_reference_order());
    return grid;
}

// The form by mean row length, at the thresholds of the fp64 choice (spmv_auto_kernel): lane = row up to 20, then 8 / 16 / 32 lanes per row.
int launch_spmv_float(hipStream_t s, const float* e32, const int* rowOffsets, const int* columnIndeces, const float* x, float* y, long long nnz, long long rows,
                      double* partials, const int* done)
{
    if (rows <= 0) return 0;
    const double avg = (double)nnz / (double)rows;
    if (avg <= 20.0) {
        const long long tiles = (rows + kBlock - 1) / kBlock;
        const int grid = (int)(tiles < kMaxGrid ? tiles : kMaxGrid);
        with_flags([&](auto DOT) {
            hipLaunchKernelGGL((spmv_float_rows_kernel<DOT.value>), dim3(grid), dim3(kBlock), 0, s, e32, rowOffsets, columnIndeces, x, y, nnz, rows, partials, done);
        }, partials != nullptr);
        return grid;
    }
    if (avg <= 28.0) return launch_spmv_float_vector<8>(s, e32, rowOffsets, columnIndeces, x, y, nnz, rows, partials, done);
    if (avg <= 128.0) return launch_spmv_float_vector<16>(s, e32, rowOffsets, columnIndeces, x, y, nnz, rows, partials, done);
    return launch_spmv_float_vector<32>(s, e32, rowOffsets, columnIndeces, x, y, nnz, rows, partials, done);
}

// ------------------------------------------------------------------ validation mode: out[0] = sum (double)x_i (double)y_i, left to right
// dot_serial_kernel (kernels_blas1.hip) for float operands: the products are exact in fp64, waves 1-3 stage a batch of them in LDS while
// lane 0 adds the batch before it in index order.
constexpr int kMixedSerialBatch = 2048;
__global__ __launch_bounds__(kBlock) void mixed_dot_serial_kernel(const float* __restrict__ x, const float* __restrict__ y, long long n, double* __restrict__ out, const int* done)
{
    __shared__ double s_prod[2][kMixedSerialBatch];
    if (done != nullptr && *done != 0) return;
    const int tid = threadIdx.x;
    const long long nBatches = (n + kMixedSerialBatch - 1) / kMixedSerialBatch;
    auto fill = [&](int buf, long long b) {
        const long long base = b * kMixedSerialBatch;
        for (int k = tid - kWave; k < kMixedSerialBatch; k += kBlock - kWave) {
            const long long i = base + k;
            s_prod[buf][k] = i < n ? (double)x[i] * (double)y[i] : 0.0;
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
            for (int k = 0; k < kMixedSerialBatch; ++k) acc += q[k];
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = acc;
}
static void launch_mixed_dot_serial(hipStream_t s, const float* x, const float* y, long long n, double* out, const int* done)
{
    hipLaunchKernelGGL(mixed_dot_serial_kernel, dim3(1), dim3(kBlock), 0, s, x, y, n < 0 ? 0 : n, out, done);
}

// ------------------------------------------------------------------ the vector passes
// Every pass walks the vectors in quads of four floats (16-byte accesses, two quads in flight per lane: chunk_pairs) and leaves the
// n % 4 last elements to the first lanes of the first workgroup, one element each.  The fp32 vectors are the library's and start on
// 16-byte boundaries; a pass that also touches the caller's x or r takes the element-wise form (V4 = false) when that vector does not.
template <typename Quad, typename One>
__device__ __forceinline__ void quad_pass(long long n, Quad quad, One one)
{
    chunk_pairs(n >> 2, [&](long long i, bool two) { quad(i); if (two) quad(i + kBlock); });
    const long long tail = n & ~3LL;
    if (blockIdx.x == 0 && tail + threadIdx.x < n) one(tail + threadIdx.x);
}
static int mixed_grid(long long n) { return grid_for(n >> 2, 2); }

// alpha = rr / pAp from the partial sums of the product ; alpha32 = (float)alpha ; r32 = r32 + ((-alpha32) * Ap32) ; partial sums of
// rn = sum (double)r_i (double)r_i.  The first lane closes the update's gate, publishes alpha and freezes what the x/p pass and the
// restart pass read in every workgroup.  p.Ap that is not finite and > 0, or an alpha32 that is not finite, leaves r32 alone and says so (fBroken).
template <bool NTV>
__global__ __launch_bounds__(kBlock) void mixed_update_r_kernel(CgScalars* __restrict__ sc, MixedScalars* __restrict__ ms, float* __restrict__ r32, const float* __restrict__ Ap32,
                                                                long long n, double* __restrict__ partials, const double* __restrict__ pApPartials, int nPAp)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) ms->gate = 1;
    if (sc->done != 0) { if (first) sc->fDone = 1; return; }           // tells the x/p pass that no iteration ran
    const double pAp = reduce_partials_block(pApPartials, nPAp, s_red, 0);
    const double rr = sc->rr;
    const double alpha = rr / pAp;
    const float alpha32 = (float)alpha;
    // (an alpha beyond the fp32 range -- a tiny positive p.Ap -- would put infinities into xs before the next update could see them)
    const bool broken = !(pAp > 0.0 && pAp <= 1.79e308) || !(fabs((double)alpha32) <= kFloatMax);
    if (first) {
        sc->pAp = pAp; sc->alpha = alpha;
        sc->fRr = rr; sc->fRr0 = sc->rr0; sc->fAlpha = alpha; sc->fIteration = sc->iteration; sc->fDone = 0;
        ms->fMaxrr = ms->maxrr; ms->fWant = ms->want; ms->fBroken = broken ? 1 : 0;
    }
    if (broken) return;
    const float malpha = -alpha32;
    double acc = 0.0;
    auto step = [&](float ap, float rv) { const float u = malpha * ap; const float v = rv + u; const double q = (double)v * (double)v; acc += q; return v; };
    f4* r4 = (f4*)r32; const f4* a4 = (const f4*)Ap32;
    quad_pass(n,
        [&](long long i) {
            const f4 av = ldv<NTV>(a4 + i); f4 rv = ldv<NTV>(r4 + i);
            rv.x = step(av.x, rv.x); rv.y = step(av.y, rv.y); rv.z = step(av.z, rv.z); rv.w = step(av.w, rv.w);
            stv<NTV>(rv, r4 + i);
        },
        [&](long long i) { r32[i] = step(Ap32[i], r32[i]); });
    const double t = block_sum(acc, s_red2);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// The x/p pass with the iteration's finalisation folded in.  Every workgroup adds the partial sums of rn in the same order and takes the
// same decisions from the frozen scalars: maxrr, the flag want, whether this iteration is an update slot, beta.  Then
// xs = xs + (alpha32 * p32) and, outside an update slot, p32 = r32 + (beta32 * p32).  The first workgroup alone publishes: outside a slot
// the iteration (trace: the recurrence's residual), in a slot only the open gate -- the restart pass publishes with the true residual.
template <bool NTV>
__global__ __launch_bounds__(kBlock) void mixed_update_xp_kernel(FinalizeArgs f, MixedScalars* __restrict__ ms, const double* __restrict__ partials, int nPartials,
                                                                 float* __restrict__ xs, float* __restrict__ p32, const float* __restrict__ r32, long long n)
{
    __shared__ double s_red[4];
    CgScalars* sc = f.sc;
    if (sc->fDone != 0) return;                                        // the loop had stopped before this iteration: nothing ran
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const int it = sc->fIteration;
    const double rr = sc->fRr, rr0 = sc->fRr0;
    if (ms->fBroken != 0) {                                            // breakdown: x keeps its last folded iterate
        if (first) {
            StopDecision d;
            d.res = sqrt(rr); d.shown = f.rule == MGCG_RULE_VIENNACL ? sqrt(rr / rr0) : d.res; d.stop = true; d.status = MGCG_NONFINITE;
            publish_iteration<0>(f, d, it, rr, 0.0, 0, [] {});
        }
        return;
    }
    const double rn = reduce_partials_block(partials, nPartials, s_red, 0);
    const double fMaxrr = ms->fMaxrr;
    const double maxrr = rn > fMaxrr ? rn : fMaxrr;
    StopDecision d = decide_stop(f, rn, 0.0, rr0, it);
    const double drop = 0.01 * maxrr;
    const bool want = ms->fWant != 0 || rn < drop || d.stop;
    const bool slot = (it & 3) == 3 && want;
    const float alpha32 = (float)sc->fAlpha;
    const double beta = rn / rr;
    const float beta32 = (float)beta;
    if (first) {
        ms->maxrr = maxrr; ms->want = want ? 1 : 0;
        if (slot) ms->gate = 0;
        else { d.stop = false; d.status = MGCG_OK; publish_iteration<0>(f, d, it, rn, 0.0, 0, [&] { sc->beta = beta; sc->rr = rn; }); }
    }
    f4* x4 = (f4*)xs; f4* p4 = (f4*)p32; const f4* r4 = (const f4*)r32;
    if (slot) {
        quad_pass(n,
            [&](long long i) {
                const f4 pv = ldv<NTV>(p4 + i); f4 xv = ldv<NTV>(x4 + i);
                const float t0 = alpha32 * pv.x, t1 = alpha32 * pv.y, t2 = alpha32 * pv.z, t3 = alpha32 * pv.w;
                xv.x = xv.x + t0; xv.y = xv.y + t1; xv.z = xv.z + t2; xv.w = xv.w + t3;
                stv<NTV>(xv, x4 + i);
            },
            [&](long long i) { const float t = alpha32 * p32[i]; xs[i] = xs[i] + t; });
        return;
    }
    quad_pass(n,
        [&](long long i) {
            f4 pv = ldv<NTV>(p4 + i); f4 xv = ldv<NTV>(x4 + i); const f4 rv = ldv<NTV>(r4 + i);
            const float t0 = alpha32 * pv.x, t1 = alpha32 * pv.y, t2 = alpha32 * pv.z, t3 = alpha32 * pv.w;
            xv.x = xv.x + t0; xv.y = xv.y + t1; xv.z = xv.z + t2; xv.w = xv.w + t3;
            const float u0 = beta32 * pv.x, u1 = beta32 * pv.y, u2 = beta32 * pv.z, u3 = beta32 * pv.w;
            pv.x = rv.x + u0; pv.y = rv.y + u1; pv.z = rv.z + u2; pv.w = rv.w + u3;
            stv<NTV>(xv, x4 + i); stv<NTV>(pv, p4 + i);
        },
        [&](long long i) { const float pv = p32[i]; const float t = alpha32 * pv; xs[i] = xs[i] + t; const float u = beta32 * pv; p32[i] = r32[i] + u; });
}

// Reliable update, first launch: x = x + (double)xs ; xs = 0.
template <bool V4, bool NTV>
__global__ __launch_bounds__(kBlock) void mixed_fold_x_kernel(const MixedScalars* __restrict__ ms, double* __restrict__ x, float* __restrict__ xs, long long n)
{
    if (ms->gate != 0) return;
    auto one = [&](long long i) { x[i] = x[i] + (double)xs[i]; xs[i] = 0.0f; };
    if constexpr (V4) {
        f4* s4 = (f4*)xs; d2* x2 = (d2*)x;
        quad_pass(n,
            [&](long long i) {
                const f4 sv = ldv<NTV>(s4 + i); d2 lo = ldv<NTV>(x2 + 2 * i), hi = ldv<NTV>(x2 + 2 * i + 1);
                lo.x = lo.x + (double)sv.x; lo.y = lo.y + (double)sv.y; hi.x = hi.x + (double)sv.z; hi.y = hi.y + (double)sv.w;
                stv<NTV>(lo, x2 + 2 * i); stv<NTV>(hi, x2 + 2 * i + 1);
                const f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
                stv<NTV>(zero, s4 + i);
            }, one);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

// Reliable update, last launch (behind r = b - A x and the partial sums of r.r): every workgroup adds the partial sums, takes the stop
// decision on the true rn -- decide_stop's text, plus MGCG_NONFINITE when sqrt(rn) is not below FLT_MAX, the range in which (float)r is
// finite -- and beta = rn / rr ; then r32 = (float)r and, unless the loop stops here, p32 = r32 + (beta32 * p32).  The first workgroup
// publishes the iteration with the true residual, hands rn over as rr and maxrr, counts the update and clears want.
template <bool V4, bool NTV>
__global__ __launch_bounds__(kBlock) void mixed_restart_kernel(FinalizeArgs f, MixedScalars* __restrict__ ms, const double* __restrict__ partials, int nPartials,
                                                               const double* __restrict__ r, float* __restrict__ r32, float* __restrict__ p32, long long n)
{
    __shared__ double s_red[4];
    if (ms->gate != 0) return;
    CgScalars* sc = f.sc;
    const double rn = reduce_partials_block(partials, nPartials, s_red, 0);
    const int it = sc->fIteration;
    StopDecision d = decide_stop(f, rn, 0.0, sc->fRr0, it);
    if (!d.stop && !(d.res < kFloatMax)) { d.stop = true; d.status = MGCG_NONFINITE; }
    const double beta = rn / sc->fRr;
    const float beta32 = (float)beta;
    const bool stop = d.stop;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ms->maxrr = rn; ms->want = 0; ms->updates = ms->updates + 1;
        publish_iteration<0>(f, d, it, rn, 0.0, 0, [&] { sc->beta = beta; sc->rr = rn; });
    }
    auto one = [&](long long i) { const float rv = (float)r[i]; r32[i] = rv; if (!stop) { const float u = beta32 * p32[i]; p32[i] = rv + u; } };
    if constexpr (V4) {
        const d2* r2 = (const d2*)r; f4* q4 = (f4*)r32; f4* p4 = (f4*)p32;
        quad_pass(n,
            [&](long long i) {
                const d2 lo = ldv<NTV>(r2 + 2 * i), hi = ldv<NTV>(r2 + 2 * i + 1);
                f4 rv; rv.x = (float)lo.x; rv.y = (float)lo.y; rv.z = (float)hi.x; rv.w = (float)hi.y;
                stv<NTV>(rv, q4 + i);
                if (!stop) {
                    f4 pv = ldv<NTV>(p4 + i);
                    const float u0 = beta32 * pv.x, u1 = beta32 * pv.y, u2 = beta32 * pv.z, u3 = beta32 * pv.w;
                    pv.x = rv.x + u0; pv.y = rv.y + u1; pv.z = rv.z + u2; pv.w = rv.w + u3;
                    stv<NTV>(pv, p4 + i);
                }
            }, one);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

// The start: rr0 = rr = maxrr = r.r from the partial sums of the residual product ; r32 = (float)r ; p32 = r32 ; xs = 0.  The first lane
// resets the scalars and the host mirror; a residual outside the float range ends the solve before its first iteration.
template <bool V4>
__global__ __launch_bounds__(kBlock) void mixed_start_kernel(FinalizeArgs f, MixedScalars* __restrict__ ms, const double* __restrict__ partials, int nPartials,
                                                             const double* __restrict__ r, float* __restrict__ r32, float* __restrict__ p32, float* __restrict__ xs, long long n)
{
    __shared__ double s_red[4];
    const double rr0 = reduce_partials_block(partials, nPartials, s_red, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        CgScalars* sc = f.sc;
        HostMirror* m = f.mirror;
        const bool bad = !(sqrt(rr0) < kFloatMax);
        sc->rr = rr0; sc->rr0 = rr0; sc->pAp = 0; sc->rrNew = 0; sc->rzNew = 0; sc->residual = sqrt(rr0); sc->nrmInf = 0; sc->beta = 0; sc->alpha = 0;
        sc->iteration = 0; sc->status = bad ? MGCG_NONFINITE : MGCG_OK; sc->pad = 0; sc->pSlot = 0;
        sc->fRr = rr0; sc->fRr0 = rr0; sc->fAlpha = 0; sc->fIteration = 0; sc->fDone = bad ? 1 : 0;
        ms->maxrr = rr0; ms->fMaxrr = rr0; ms->want = 0; ms->fWant = 0; ms->gate = 1; ms->updates = 0; ms->fBroken = 0;
        m->residual = sqrt(rr0); m->iteration = 0; m->status = sc->status;
        sc->done = bad ? 1 : 0;
        __threadfence_system();
        m->done = bad ? 1 : 0;
    }
    auto one = [&](long long i) { const float rv = (float)r[i]; r32[i] = rv; p32[i] = rv; xs[i] = 0.0f; };
    if constexpr (V4) {
        const d2* r2 = (const d2*)r; f4* q4 = (f4*)r32; f4* p4 = (f4*)p32; f4* s4 = (f4*)xs;
        quad_pass(n,
            [&](long long i) {
                const d2 lo = r2[2 * i], hi = r2[2 * i + 1];
                f4 rv; rv.x = (float)lo.x; rv.y = (float)lo.y; rv.z = (float)hi.x; rv.w = (float)hi.y;
                const f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
                q4[i] = rv; p4[i] = rv; s4[i] = zero;
            }, one);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

void mixed_enqueue_start(const MixedRun& R, const FinalizeArgs& f, int nPartials)
{
    hipStream_t s = R.ws->stream;
    with_flags([&](auto V4) {
        hipLaunchKernelGGL((mixed_start_kernel<V4.value>), dim3(V4.value ? mixed_grid(R.n) : grid_for(R.n, 1)), dim3(kBlock), 0, s, f, R.ws->mixedScalars,
                           (const double*)R.ws->partials, nPartials, (const double*)R.r, R.r32, R.p32, R.xs, R.n);
    }, al16(R.r));
}

bool mixed_enqueue_iteration(const MixedRun& R, const FinalizeArgs& f)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    CgScalars* sc = ws->scalars;
    const int* done = &sc->done;
    const bool serial = dot_reference_order();
    const bool nt = vec_nt(R.n);
    double* rrPartials = ws->partials + 2 * kMaxPartials;              // (the plain loop's regions: p.Ap in the first, the r pass's sums in the third)
    int nPAp = launch_spmv_float(s, R.e32, R.rowOffsets, R.columnIndeces, R.p32, R.Ap32, R.nnz, R.n, ws->partials, done);
    if (serial) { launch_mixed_dot_serial(s, R.p32, R.Ap32, R.n, ws->partials, done); nPAp = 1; }
    // two workgroups per CU for the 2-reads-1-write r pass, as update_r_kernel's; the x/p pass keeps the full grid
    int gridR = mixed_grid(R.n);
    { DeviceState* d = device_state(); const int want = 2 * (d ? d->numCu : kNumCu); if (gridR > want) gridR = want; }
    with_flags([&](auto NTV) {
        hipLaunchKernelGGL((mixed_update_r_kernel<NTV.value>), dim3(gridR), dim3(kBlock), 0, s, sc, ws->mixedScalars, R.r32, (const float*)R.Ap32, R.n, rrPartials,
                           (const double*)ws->partials, nPAp);
    }, nt);
    int nRn = gridR;
    if (serial) { launch_mixed_dot_serial(s, R.r32, R.r32, R.n, rrPartials, done); nRn = 1; }
    with_flags([&](auto NTV) {
        hipLaunchKernelGGL((mixed_update_xp_kernel<NTV.value>), dim3(mixed_grid(R.n)), dim3(kBlock), 0, s, f, ws->mixedScalars, (const double*)rrPartials, nRn,
                           R.xs, R.p32, (const float*)R.r32, R.n);
    }, nt);
    return MGCG_HIP(hipGetLastError());
}

void mixed_enqueue_fold(const MixedRun& R)
{
    hipStream_t s = R.ws->stream;
    with_v2_nt(al16(R.x), vec_nt(R.n), [&](auto V4, auto NTV) {
        hipLaunchKernelGGL((mixed_fold_x_kernel<V4.value, NTV.value>), dim3(V4.value ? mixed_grid(R.n) : grid_for(R.n, 1)), dim3(kBlock), 0, s,
                           (const MixedScalars*)R.ws->mixedScalars, R.x, R.xs, R.n);
    });
}

void mixed_enqueue_restart(const MixedRun& R, const FinalizeArgs& f, int nPartials)
{
    hipStream_t s = R.ws->stream;
    with_v2_nt(al16(R.r), vec_nt(R.n), [&](auto V4, auto NTV) {
        hipLaunchKernelGGL((mixed_restart_kernel<V4.value, NTV.value>), dim3(V4.value ? mixed_grid(R.n) : grid_for(R.n, 1)), dim3(kBlock), 0, s, f, R.ws->mixedScalars,
                           (const double*)R.ws->partials, nPartials, (const double*)R.r, R.r32, R.p32, R.n);
    });
}

void preload_kernels_mixed() { preload_code_object(reinterpret_cast<const void*>(&mixed_convert_kernel)); }

} // namespace mgcg

using namespace mgcg;

extern "C" {

int MgcgMixedSetup(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   int elementsCount, int count, Vector* elements32Vector, int* exact)
{
    if (!cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector || !elements32Vector) { set_error("MgcgMixedSetup: null handle"); return -1; }
    if (elementsCount < 0 || count < 0) { set_error("MgcgMixedSetup: bad sizes"); return -1; }
    if (elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount || rowOffsetsVector->size < (long long)count + 1) {
        set_error("MgcgMixedSetup: a device vector is smaller than the matrix"); return -1;
    }
    if (elements32Vector->size < ((long long)elementsCount + 1) / 2) {
        set_error("MgcgMixedSetup: the elements32 vector holds %lld doubles, %d floats need %lld", elements32Vector->size, elementsCount, ((long long)elementsCount + 1) / 2);
        return -1;
    }
    if (!device_state()) return -1;
    if (exact) *exact = 1;
    if (elementsCount == 0) return 0;
    hipStream_t s = cusparse->ws.stream;
    int* flags = cusparse->ws.devInts + 5;                             // {rounded, not finite, first such row}
    int h3[3] = { 0, 0, 0x7fffffff };
    analysis_note_write(elements32Vector->data, sizeof(float) * (size_t)elementsCount);
    bool ok = MGCG_HIP(hipMemcpyAsync(flags, h3, sizeof(h3), hipMemcpyHostToDevice, s));
    if (ok) launch_mixed_convert(s, elementsVector->data, rowOffsetsVector->data, elementsCount, count, (float*)elements32Vector->data, flags);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(h3, flags, sizeof(h3), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));   // the one read-back
    if (!ok) return -1;
    if (exact) *exact = h3[0] == 0 ? 1 : 0;
    if (h3[1] == 0) return 0;
    set_error("MgcgMixedSetup: row %d holds a value that is not finite as a float (the fp32 range ends at 3.4e38)", h3[2]);
    return -1;
}

void CsrMVFloat(MgcgSparse* cusparse, MgcgMatDescr* matDescr, float* y, const float* elements32, const int* rowOffsets,
                const int* columnIndeces, const float* x, int elementsCount, int count)
{
    (void)matDescr;
    if (!device_state()) return;
    if (!cusparse || !y || !rowOffsets || !x || (elementsCount > 0 && (!elements32 || !columnIndeces))) { set_error("CsrMVFloat: null argument"); return; }
    if (count < 0 || elementsCount < 0) { set_error("CsrMVFloat: negative size"); return; }
    if (count == 0) return;
    analysis_note_write(y, sizeof(float) * (size_t)count);
    (void)launch_spmv_float(cusparse->ws.stream, elements32, rowOffsets, columnIndeces, x, y, elementsCount, count, nullptr, nullptr);
    (void)MGCG_HIP(hipGetLastError());
}

} // extern "C"
