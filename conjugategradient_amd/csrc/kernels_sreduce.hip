// Single-reduction CG for gfx950 (SolveSingleReduce / SolveSingleReduceParallel): the Chronopoulos-Gear form of CG, with the product in
// front of both sums, so that an iteration has ONE reduction point.  include/MgcgGpu.h has the method and its rounding contract.
//
// Per body k, behind the product w = A u (launch_spmv_auto with the EPI_DOT epilogue: the partial sums of delta = w.u) this file's one
// pass does everything else:
//     scalars   k = 0: beta = 0, alpha = gamma / delta;  k > 0: beta = gamma / gamma_old, t = beta gamma, q = t / alpha_old, den = delta - q,
//               alpha = gamma / den
//     vectors   p = u + beta p ; s = w + beta s ; x = x + alpha p ; r = r + (-alpha) s ; u = dinv r     (k = 0: p = u, s = w, nothing read)
//     sums      the partial sums of gamma = r.u and rr = r.r of the new r leave with the pass
// One rank: EVERY workgroup of the pass adds the product's partial sums of delta and the previous pass's partial sums of gamma and rr in one
// fixed order (reduce_partials_block, as update_r_kernel does with p.Ap), so all workgroups compute the same beta and alpha and take the
// same stop decision; the first workgroup alone persists the scalars, the trace entry and the host mirror.  What a pass reads (gamma_old,
// alpha_old, its input partial sums) and what it writes live in different slots, alternated by the parity of k: no workgroup can read what
// another has already overwritten.  The pass's own partial sums go to the second and third region of the workspace's buffer, never to the
// first, which the next product's epilogue fills.  An iteration is two launches.
// Several ranks (GIVEN): one small launch adds the three sets of partial sums into three adjacent scalars, one all-reduce carries them, and
// the pass takes them as given: three launches and one all-reduce where the plain loop has five and two.  A rank without rows launches the
// pass with one workgroup: it does the scalar step and publishes, as every other rank does.
//
// The stop decision on body k's rr is taken where the sum is known, in the pass of body k + 1: a stopping pass changes no vector, so x is
// the iterate whose residual was judged, and one product at the very end is wasted (as CgUpdate::PrecondRanks accepts, solver.hip).
// The stop flag is CgScalars::done, set by the first workgroup of the pass that stops.  A workgroup of the SAME pass may or may not see it
// up (it reads it once, through LDS, so that all its lanes agree): either it returns at its first line or it takes the same decision from
// the same sums and returns a few lines later -- no vector is touched in either case.
//
// u is never read: the old u_i is dinv_i * r_i again, the bits that were stored.  Without dinv u IS r, so during the loop the residual
// lives in the rows' slice of the full-length buffer that the product gathers from, and the pass streams 9 vectors (p, s, w, x, r in;
// p, s, x, r out: 72 bytes per row); with dinv 11 (dinv in, u out: 88).  Same grid, chunked 16-byte accesses and streaming hints as
// update_xp_final_kernel (vec_passes.hpp).
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_sreduce()
{
    if (sreduceScalars) return true;
    return MGCG_HIP(hipMalloc((void**)&sreduceScalars, sizeof(SreduceScalars)));
}

struct SreducePass {
    FinalizeArgs f;
    SreduceScalars* ss;
    const double* deltaPartials; int nDelta;          // the product's epilogue (one rank)
    const double* inRR; const double* inG; int nIn;   // the previous pass's partial sums (one rank; inG: with dinv only)
    double* outRR; double* outG;                      // this pass's
    int k;                                            // the body's index: the host's count, which is the device's while the loop is live
    double *x, *p, *s, *r, *u;                        // r: where the residual lives (without dinv the rows' slice of the full-length buffer); u: with dinv only
    const double* w; const double* dinv;
    long long n;
};

template <bool V2, bool NTV, bool DINV, bool GIVEN>
__global__ __launch_bounds__(kBlock) void sreduce_pass_kernel(SreducePass a)
{
    __shared__ double s_red[4], s_red2[4], s_red3[4], s_red4[4], s_red5[4];
    __shared__ int s_done;
    CgScalars* sc = a.f.sc;
    if (threadIdx.x == 0) s_done = sc->done;
    __syncthreads();
    if (s_done != 0) return;
    double delta, rr, gamma;
    if constexpr (GIVEN) {
        delta = a.ss->red[0]; rr = a.ss->red[1]; gamma = rr;
        if constexpr (DINV) gamma = a.ss->red[2];
    } else {
        delta = reduce_partials_block(a.deltaPartials, a.nDelta, s_red, 0);
        rr = reduce_partials_block(a.inRR, a.nIn, s_red2, 0);
        gamma = rr;
        if constexpr (DINV) gamma = reduce_partials_block(a.inG, a.nIn, s_red3, 0);
    }
    const int k = a.k;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const double rr0 = sc->rr0;
    // the residual of the last completed iterate, as the trace shows it (what a breakdown in body 0 reports)
    StopDecision d;
    d.res = sqrt(rr); d.shown = a.f.rule == MGCG_RULE_VIENNACL ? sqrt(rr / rr0) : d.res; d.stop = false; d.status = MGCG_OK;
    if (k > 0) {                                       // body k - 1's stop decision, the same in every lane of every workgroup
        d = decide_stop(a.f, rr, 0.0, rr0, k - 1);
        if (publisher) publish_iteration<0>(a.f, d, k - 1, rr, 0.0, 0, [] {});
        if (d.stop) return;
    }
    const double gammaOld = a.ss->st[k & 1].gamma, alphaOld = a.ss->st[k & 1].alpha;
    double beta = 0.0, den = delta;
    if (k > 0) { beta = gamma / gammaOld; const double t = beta * gamma; const double q = t / alphaOld; den = delta - q; }
    const double alpha = gamma / den;
    if (!(den > 0.0 && den <= kFiniteMax) || !(fabs(alpha) <= kFiniteMax)) {   // breakdown: before this body's updates
        if (publisher) { d.stop = true; d.status = MGCG_NONFINITE; publish_iteration<0>(a.f, d, k, rr, 0.0, 0, [] {}); }
        return;
    }
    if (publisher) { a.ss->st[(k + 1) & 1].gamma = gamma; a.ss->st[(k + 1) & 1].alpha = alpha; sc->alpha = alpha; sc->beta = beta; }

    const bool first = k == 0;
    const double malpha = -alpha;
    double accR = 0.0, accG = 0.0;
    // one element; e.p, e.s: the old p and s (not looked at when first), e.r the old r.  Every product into a double of its own, then the add.
    struct Elem { double p, s, x, r, u, w, d; };
    auto step = [&](Elem& e) {
        double uo = e.r;
        if constexpr (DINV) uo = e.d * e.r;
        if (first) { e.p = uo; e.s = e.w; }
        else { double bp = beta * e.p; e.p = uo + bp; double bs = beta * e.s; e.s = e.w + bs; }
        double ap = alpha * e.p; e.x = e.x + ap;
        double as = malpha * e.s; e.r = e.r + as;
        if constexpr (DINV) { e.u = e.d * e.r; double g = e.r * e.u; accG += g; }
        double q = e.r * e.r; accR += q;
    };
    auto one = [&](long long i) {
        Elem e = { 0.0, 0.0, a.x[i], a.r[i], 0.0, a.w[i], 0.0 };
        if (!first) { e.p = a.p[i]; e.s = a.s[i]; }
        if constexpr (DINV) e.d = a.dinv[i];
        step(e);
        a.p[i] = e.p; a.s[i] = e.s; a.x[i] = e.x; a.r[i] = e.r;
        if constexpr (DINV) a.u[i] = e.u;
    };
    if constexpr (V2) {
        d2* p2 = (d2*)a.p; d2* s2 = (d2*)a.s; d2* x2 = (d2*)a.x; d2* r2 = (d2*)a.r; d2* u2 = (d2*)a.u;
        const d2* w2 = (const d2*)a.w; const d2* dv2 = (const d2*)a.dinv;
        struct Pair { d2 p, s, x, r, w, d; };
        auto load = [&](Pair& v, long long i) {
            v.p = {}; v.s = {}; v.d = {};
            if (!first) { v.p = ldv<NTV>(p2 + i); v.s = ldv<NTV>(s2 + i); }
            v.w = ldv<NTV>(w2 + i); v.x = ldv<NTV>(x2 + i); v.r = ldv<NTV>(r2 + i);
            if constexpr (DINV) v.d = ldv<NTV>(dv2 + i);
        };
        auto finish = [&](const Pair& v, long long i) {
            Elem e0 = { v.p.x, v.s.x, v.x.x, v.r.x, 0.0, v.w.x, v.d.x }, e1 = { v.p.y, v.s.y, v.x.y, v.r.y, 0.0, v.w.y, v.d.y };
            step(e0); step(e1);
            d2 o;
            o.x = e0.p; o.y = e1.p; stv<NTV>(o, p2 + i);
            o.x = e0.s; o.y = e1.s; stv<NTV>(o, s2 + i);
            o.x = e0.x; o.y = e1.x; stv<NTV>(o, x2 + i);
            o.x = e0.r; o.y = e1.r; stv<NTV>(o, r2 + i);
            if constexpr (DINV) { o.x = e0.u; o.y = e1.u; stv<NTV>(o, u2 + i); }
        };
        chunk_pairs(a.n >> 1, [&](long long i, bool two) {
            const long long j = two ? i + kBlock : i;
            Pair v0, v1;
            load(v0, i); load(v1, j);
            finish(v0, i);
            if (two) finish(v1, j);
        });
        if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(a.n - 1);
    } else {
        grid_stride<false>(a.n, [&](long long) {}, one);
    }
    const double tr = block_sum(accR, s_red4);
    if (threadIdx.x == 0) a.outRR[blockIdx.x] = tr;
    if constexpr (DINV) {
        const double tg = block_sum(accG, s_red5);
        if (threadIdx.x == 0) a.outG[blockIdx.x] = tg;
    }
}

// Several ranks: this rank's {delta, rr, gamma} in red[0..2] ({delta, rr} without dinv), each sum in reduce_kernel's order
template <bool DINV>
__global__ __launch_bounds__(kBlock) void sreduce_sums_kernel(const double* __restrict__ deltaPartials, int nDelta, const double* __restrict__ inRR,
                                                              const double* __restrict__ inG, int nIn, double* __restrict__ red, const int* done)
{
    __shared__ double s_red[4], s_red2[4], s_red3[4];
    if (*done != 0) return;
    const double delta = reduce_partials_block(deltaPartials, nDelta, s_red, 0);
    const double rr = reduce_partials_block(inRR, nIn, s_red2, 0);
    double gamma = 0.0;
    if constexpr (DINV) gamma = reduce_partials_block(inG, nIn, s_red3, 0);
    if (threadIdx.x == 0) { red[0] = delta; red[1] = rr; if constexpr (DINV) red[2] = gamma; }
}

// The partial sums of a pass of parity q: rr at the start of region 1 + q of the workspace's buffer, gamma kMaxGrid doubles behind it (a pass
// has at most kMaxGrid workgroups, and so has the start's copy_dot, whose sums go where body 0 looks: parity 1).
double* sreduce_rr_partials(Workspace* ws, int parity) { return ws->partials + (size_t)(1 + (parity & 1)) * kMaxPartials; }
double* sreduce_gamma_partials(Workspace* ws, int parity) { return sreduce_rr_partials(ws, parity) + kMaxGrid; }
static_assert(2 * kMaxGrid <= kMaxPartials, "rr and gamma partial sums of one parity share a region");

void sreduce_enqueue_sums(const SreduceRun& R, int k, int nDelta, int nIn)
{
    Workspace* ws = R.ws;
    with_flags([&](auto DINV) {
        hipLaunchKernelGGL((sreduce_sums_kernel<DINV.value>), dim3(1), dim3(kBlock), 0, ws->stream, ws->partials, nDelta, sreduce_rr_partials(ws, k + 1),
                           sreduce_gamma_partials(ws, k + 1), nIn, ws->sreduceScalars->red, &ws->scalars->done);
    }, R.dinv != nullptr);
}

int sreduce_enqueue_pass(const SreduceRun& R, const FinalizeArgs& f, int k, int nDelta, int nIn)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const bool dinv = R.dinv != nullptr;
    SreducePass a{};
    a.f = f; a.ss = ws->sreduceScalars;
    a.deltaPartials = ws->partials; a.nDelta = nDelta;
    a.inRR = sreduce_rr_partials(ws, k + 1); a.inG = sreduce_gamma_partials(ws, k + 1); a.nIn = nIn;
    a.outRR = sreduce_rr_partials(ws, k); a.outG = sreduce_gamma_partials(ws, k);
    a.k = k;
    a.x = R.x; a.p = R.p; a.s = R.s; a.r = dinv ? R.r : R.u; a.u = R.u; a.w = R.w; a.dinv = R.dinv; a.n = R.n;
    const bool v2 = al16(a.x) && al16(a.p) && al16(a.s) && al16(a.r) && al16(a.u) && al16(a.w) && al16(a.dinv);
    // the grid of update_xp_final_kernel; a rank without rows: one workgroup, for the scalar step
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto DINV, auto GIVEN) {
            hipLaunchKernelGGL((sreduce_pass_kernel<V2.value, NTV.value, DINV.value, GIVEN.value>), dim3(grid), dim3(kBlock), 0, s, a);
        }, dinv, R.given);
    });
    if (dot_reference_order()) {                                       // the sums in the reference's order replace the partial sums
        launch_dot_serial(s, a.r, a.r, R.n, a.outRR, &ws->scalars->done);
        if (dinv) launch_dot_serial(s, a.r, a.r, R.n, a.outG, &ws->scalars->done, R.dinv);    // terms r_i * (dinv_i * r_i) = r_i * u_i
        return 1;
    }
    return grid;
}

void preload_kernels_sreduce() { preload_code_object(reinterpret_cast<const void*>(&sreduce_sums_kernel<false>)); }

} // namespace mgcg
