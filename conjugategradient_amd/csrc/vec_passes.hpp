// Device and launch helpers shared by the translation units that hold the vector passes of the CG loop (kernels_blas1.hip, kernels_shift.hip)
// and of the Krylov variants (kernels_sreduce, _minres, _pminres, _bicgstab, _bicgstabl, _gmres, _cheb .hip): the wavefront / workgroup
// reductions, the grid and alignment rules, the streaming-hint loads and stores, the element drivers, the fixed-order sum of per-workgroup
// partial sums, the finite tests, and what a loop's start, a finished iteration and a breakdown publish.  One definition, so that every pass
// adds in the same order, takes the same forms at the same sizes and words a stop the same way.
#pragma once
#include "common.hpp"

namespace mgcg {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum_b(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max_b(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { double o = __shfl_down(v, off, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ double block_sum(double v, double* s_red)
{
    v = wave_sum_b(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
__device__ __forceinline__ double block_max(double v, double* s_red)
{
    v = wave_max_b(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = s_red[0] > s_red[1] ? s_red[0] : s_red[1];
    double b = s_red[2] > s_red[3] ? s_red[2] : s_red[3];
    return a > b ? a : b;
}

static inline int grid_for(long long n, int perThread)
{
    const int cap = kMaxGrid;
    long long blocks = (n + (long long)kBlock * perThread - 1) / ((long long)kBlock * perThread);
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Element-wise grid-stride driver.  V2: f2(i) handles elements i, i+1 with 16-byte accesses and the
// odd tail goes to f1 on one thread; otherwise f1(i) per element.
// Streaming hint of the CG vector passes (non-temporal loads and stores).  Measured per size, alternating inside one process
// (profiles/r2/vec_nt_ab.log; the A/B script is in the history): with the hint the CG iteration is 2-11 % faster from 4 M rows up (11 % at the 16.8 M rows
// of one rank's slab of an 8-GPU run, 2 % at 134 M) and 2.5 % slower at 2 M rows and below, where every vector stays in the caches anyway.
template <bool NTV, typename T> __device__ __forceinline__ T ldv(const T* p) { if constexpr (NTV) return __builtin_nontemporal_load(p); else return *p; }
template <bool NTV, typename T> __device__ __forceinline__ void stv(const T& v, T* p) { if constexpr (NTV) __builtin_nontemporal_store(v, p); else *p = v; }
static inline bool vec_nt(long long n) { return n > 3000000; }

// Run-time flags to template arguments: go(std::bool_constant<flag>...).  The kernels' launches name every form they instantiate here.
template <typename Go> static void with_flags(Go go) { go(); }
template <typename Go, typename... Rest> static void with_flags(Go go, bool flag, Rest... rest)
{
    if (flag) with_flags([&](auto... c) { go(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { go(std::false_type{}, c...); }, rest...);
}
// The three forms of the loop's x/p passes, go(V2, NTV): 16-byte accesses with the streaming hint, without it, or one element at a time.
template <typename Go> static void with_v2_nt(bool v2, bool nt, Go go)
{
    if (v2 && nt) go(std::true_type{}, std::true_type{});
    else if (v2) go(std::true_type{}, std::false_type{});
    else go(std::false_type{}, std::false_type{});
}

// Who forms the hatted copy hat(v) = M^-1 v of a BiCGStab or BiCGStab(l) pass: nobody (M = I: the vector itself is read), the pass (dinv *
// value per element), or somebody else between the passes (the V-cycle: the copy is stored, the passes only read it).  go(HAT); a loop
// without a stored form passes no `stored` and instantiates none.
enum : int { HAT_NONE = 0, HAT_DINV = 1, HAT_STORED = 2 };
template <typename Go> static void with_hat(const double* dinv, Go go)
{
    if (dinv) go(std::integral_constant<int, HAT_DINV>{});
    else go(std::integral_constant<int, HAT_NONE>{});
}
template <typename Go> static void with_hat(const double* dinv, bool stored, Go go)
{
    if (dinv) go(std::integral_constant<int, HAT_DINV>{});
    else if (stored) go(std::integral_constant<int, HAT_STORED>{});
    else go(std::integral_constant<int, HAT_NONE>{});
}

template <bool V2, typename F2, typename F1>
__device__ __forceinline__ void grid_stride(long long n, F2 f2, F1 f1)
{
    const long long stride = (long long)gridDim.x * kBlock;
    if constexpr (V2) {
        const long long n2 = n >> 1;
        for (long long i2 = (long long)blockIdx.x * kBlock + threadIdx.x; i2 < n2; i2 += stride) f2(i2 * 2);
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) f1(n - 1);
    } else {
        for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) f1(i);
    }
}

// Contiguous-chunk driver for the loop's own vector updates: workgroup b walks its own run of element pairs, two
// 16-byte accesses per array in flight per lane.  Measured 8-15 % faster than the grid-stride form on the 1 GiB vectors
// of the 512^3 system (profiles/r1/vec_probe_update_kernels.log); same arithmetic per element.
template <typename F2>
__device__ __forceinline__ void chunk_pairs(long long n2, F2 f2x2)
{
    const long long per = ((n2 + gridDim.x - 1) / gridDim.x + (kBlock - 1)) & ~(long long)(kBlock - 1);
    long long i = per * blockIdx.x + threadIdx.x;
    long long end = per * (blockIdx.x + 1);
    end = end < n2 ? end : n2;
    for (; i < end; i += 2 * kBlock) f2x2(i, i + kBlock < end);    // pairs i and i + kBlock
}

// The chunked 16-byte driver of the Krylov variants' passes: load(e, i) fills a Pair for pair index i, finish(e, i) computes and stores it,
// one(i) is the element-wise form.  Two pairs per array in flight per lane; the odd tail goes to the first thread (publisher).
template <bool V2, typename Pair, typename Load, typename Finish, typename One>
__device__ __forceinline__ void stream_pairs(long long n, bool publisher, Load load, Finish finish, One one)
{
    if constexpr (V2) {
        chunk_pairs(n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            Pair e0, e1;
            load(e0, i); load(e1, j);
            finish(e0, i);
            if (two) finish(e1, j);
        });
        if ((n & 1) && publisher) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

// The tests of a scalar that a loop divides by or judges: neither infinite nor NaN; and that, above zero.  kFiniteMax: the bound of both,
// for the one test that is neither (a sum that may be zero but not negative).
constexpr double kFiniteMax = 1.79e308;
__device__ __forceinline__ bool finite_value(double v) { return fabs(v) <= kFiniteMax; }
__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v <= kFiniteMax; }

// Fixed-order sum (or max) of n partials by the whole workgroup.  The result is valid in EVERY thread: block_sum / block_max read s_red in
// all threads behind their barrier (update_shifted_kernel relies on it in lanes 0 .. K-1; the other callers use thread 0's copy).
__device__ __forceinline__ double reduce_partials_block(const double* __restrict__ partials, int n, double* s_red, int mode)
{
    double acc = 0.0;
    if (mode == 0) { for (int i = threadIdx.x; i < n; i += kBlock) acc += partials[i]; return block_sum(acc, s_red); }
    for (int i = threadIdx.x; i < n; i += kBlock) { double a = partials[i]; acc = a > acc ? a : acc; }
    return block_max(acc, s_red);
}

// What a finished iteration publishes, by one thread: the trace entry, the live scalars, the host mirror (its `done` last, behind a
// system-wide fence).  pad: 1 when this iteration's x += alpha p is still to be done by update_xp_kernel.  RING_NT > 0 (deferred x update):
// the iteration that stops the loop also records the slot that holds p.  `next` hands beta and r.r (or r.z) over to the next iteration:
// the callers differ in where they take them from.
template <int RING_NT, typename Next>
__device__ __forceinline__ void publish_iteration(const FinalizeArgs& f, const StopDecision& d, int it, double rrNew, double inf, int pad, Next next)
{
    CgScalars* sc = f.sc;
    if (f.trace != nullptr && it < f.traceCap) f.trace[it] = d.shown;
    sc->rrNew = rrNew; sc->residual = d.res; sc->nrmInf = inf; sc->pad = pad;
    if (d.stop) {
        if constexpr (RING_NT > 0) sc->pSlot = RING_NT - 1;           // p_k stays where it is (ring_copy_back_kernel)
        sc->done = 1; sc->status = d.status;
        f.mirror->residual = d.res; f.mirror->iteration = it; f.mirror->status = d.status;
        __threadfence_system();
        f.mirror->done = 1;
    } else {
        next();
        sc->iteration = it + 1;
        f.mirror->residual = d.res; f.mirror->iteration = it + 1;
    }
}

// The start of a variant's loop, by one thread: every field of CgScalars, the host mirror and trace[0] for the first judged figure rr0 (r.r,
// or r.z of a preconditioned recurrence) and the residual res0 that goes with it.  The loop's own scalars follow it, and then, where rr0 is
// zero or not finite (b - A x is), refuse_start: the loop ends MGCG_NONFINITE at iteration 0.
__device__ __forceinline__ void publish_start(const FinalizeArgs& f, double rr0, double res0)
{
    CgScalars* sc = f.sc;
    sc->rr = rr0; sc->rr0 = rr0; sc->pAp = 0; sc->rrNew = rr0; sc->rzNew = 0; sc->residual = res0; sc->nrmInf = 0;
    sc->beta = 0; sc->alpha = 0; sc->iteration = 0; sc->done = 0; sc->status = MGCG_OK; sc->pad = 0;
    sc->fRr = rr0; sc->fRr0 = rr0; sc->fAlpha = 0; sc->fIteration = 0; sc->fDone = 0; sc->pSlot = 0;
    f.mirror->residual = res0; f.mirror->iteration = 0; f.mirror->status = MGCG_OK; f.mirror->done = 0;
    if (f.trace != nullptr && f.traceCap > 0) f.trace[0] = f.rule == MGCG_RULE_VIENNACL ? sqrt(rr0 / rr0) : res0;
}
__device__ __forceinline__ void refuse_start(const FinalizeArgs& f)
{
    f.sc->done = 1; f.sc->status = MGCG_NONFINITE;
    f.mirror->status = MGCG_NONFINITE;
    __threadfence_system();
    f.mirror->done = 1;
}

// A breakdown in front of an iteration's updates, by one thread: the last judged residual once more, for iteration `it`
__device__ __forceinline__ void publish_breakdown(const FinalizeArgs& f, int it)
{
    StopDecision d;
    const double rrOld = f.sc->rrNew, rr0 = f.sc->rr0;
    d.res = sqrt(rrOld); d.shown = f.rule == MGCG_RULE_VIENNACL ? sqrt(rrOld / rr0) : d.res; d.stop = true; d.status = MGCG_NONFINITE;
    publish_iteration<0>(f, d, it, rrOld, 0.0, 0, [] {});
}

} // namespace mgcg
