// MINRES for gfx950 (SolveMinres / SolveMinresParallel): Paige and Saunders' minimum-residual method for (A - shift I) x = b with A symmetric,
// definite or not.  include/MgcgGpu.h has the method and its rounding contract; solver.hip's cg_solve_minres the host's side.
//
// Per body k, behind the product q = A v (launch_spmv_auto with the EPI_DOT epilogue: the partial sums of delta = v.q), two passes:
//     pass A  minres_lanczos_kernel   y = (q - delta v) - beta vprev, in place over vprev, and the partial sums of y.y     (3 reads, 1 write: 32 bytes per row)
//     pass B  minres_update_kernel    the Givens rotation from (delta - shift, sqrt(y.y)) and the state of the body before, the stop decision on
//                                     |phibar|, then w = ((v - oldeps w1) - dl w2) / gamma over w1, x = x + phi w, vnext = y / betan over y
//                                                                                                                           (5 reads, 3 writes: 64 bytes per row)
// An iteration is three launches with two reduction points.  The shift enters the scalar alpha = delta - shift only: the Lanczos vectors of
// A - shift I are those of A.  The host rotates (vprev, v) and (w1, w2) by swapping two pointer pairs; nothing is copied or allocated per body.
// One rank: EVERY workgroup of pass A adds the product's partial sums of delta in one fixed order (reduce_partials_block) and its first
// workgroup leaves delta in MinresScalars::red[0] for pass B; every workgroup of pass B adds pass A's partial sums of y.y the same way, so all
// of them compute the same rotation and take the same stop decision, and the first alone persists the state, the trace entry and the host
// mirror.  What a body reads (st[k & 1]) and what it writes (st[(k + 1) & 1]) are different slots, as in kernels_sreduce.hip.
// Several ranks (GIVEN): delta and y.y are folded by one small launch each (launch_reduce_to), all-reduced in place in red[0] and red[1], and
// the passes take them as given.  A rank without rows launches both passes with one workgroup for the scalar steps.
//
// The stop flag is CgScalars::done.  Unlike the single-reduction pass, the pass that stops the loop DOES change vectors (x of the judged
// iterate), so its workgroups must not look at a flag that one of them raises: pass A, which raises nothing, copies the flag as it found it
// into MinresScalars::fDone, and pass B looks there.  Bodies enqueued behind a raised flag return at their first instruction.
//
// Same grid, chunked 16-byte accesses and streaming hints as update_xp_final_kernel and sreduce_pass_kernel (vec_passes.hpp).
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_minres()
{
    if (minresScalars) return true;
    return MGCG_HIP(hipMalloc((void**)&minresScalars, sizeof(MinresScalars)));
}

// pass A's partial sums of y.y (and the start's and closing pass's of r.r): the second region of the workspace's buffer, never the first,
// which the product's epilogue fills
double* minres_yy_partials(Workspace* ws) { return ws->partials + kMaxPartials; }
static_assert(kMaxGrid <= kMaxPartials, "a pass has at most kMaxGrid workgroups");

struct MinresPass {
    FinalizeArgs f;
    MinresScalars* ms;
    const double* inPartials; int nIn;                // pass A: the product's partial sums of delta; pass B: pass A's of y.y (one rank)
    double* outPartials;                              // pass A: y.y
    int k;                                            // the body's index: the host's count, which is the device's while the loop is live
    double shift;
    double *x, *y, *w1;                               // y: the vprev buffer (pass A writes y there, pass B vnext); w1: pass B writes w there
    const double *q, *v, *w2;
    long long n;
};

template <bool V2, bool NTV, bool GIVEN>
__global__ __launch_bounds__(kBlock) void minres_lanczos_kernel(MinresPass a)
{
    __shared__ double s_red[4], s_red2[4];
    const int done = a.f.sc->done;                     // nobody writes it while this pass runs
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (publisher) a.ms->fDone = done;
    if (done != 0) return;
    double delta;
    if constexpr (GIVEN) delta = a.ms->red[0];
    else {
        delta = reduce_partials_block(a.inPartials, a.nIn, s_red, 0);
        if (publisher) a.ms->red[0] = delta;
    }
    const bool first = a.k == 0;
    const double beta = a.ms->st[a.k & 1].beta;
    double acc = 0.0;
    // one element: every product into a double of its own, then the subtraction
    auto step = [&](double q, double v, double vp) {
        double dv = delta * v; double y = q - dv;
        if (!first) { double bv = beta * vp; y = y - bv; }
        double t = y * y; acc += t;
        return y;
    };
    auto one = [&](long long i) { a.y[i] = step(a.q[i], a.v[i], first ? 0.0 : a.y[i]); };
    const d2* q2 = (const d2*)a.q; const d2* v2 = (const d2*)a.v; d2* y2 = (d2*)a.y;
    struct Pair { d2 q, v, p; };
    auto load = [&](Pair& e, long long i) { e.p = {}; e.q = ldv<NTV>(q2 + i); e.v = ldv<NTV>(v2 + i); if (!first) e.p = ldv<NTV>(y2 + i); };
    auto finish = [&](const Pair& e, long long i) { d2 o; o.x = step(e.q.x, e.v.x, e.p.x); o.y = step(e.q.y, e.v.y, e.p.y); stv<NTV>(o, y2 + i); };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    const double t = block_sum(acc, s_red2);
    if (threadIdx.x == 0) a.outPartials[blockIdx.x] = t;
}

template <bool V2, bool NTV, bool GIVEN>
__global__ __launch_bounds__(kBlock) void minres_update_kernel(MinresPass a)
{
    __shared__ double s_red[4];
    if (a.ms->fDone != 0) return;                      // the flag as pass A found it: this pass raises the live one itself
    const double delta = a.ms->red[0];
    double yy;
    if constexpr (GIVEN) yy = a.ms->red[1];
    else yy = reduce_partials_block(a.inPartials, a.nIn, s_red, 0);
    const int k = a.k;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const MinresScalars::State st = a.ms->st[k & 1];
    const double rr0 = a.f.sc->rr0;
    // the rotation, every product rounded before the add or subtraction that follows it, in the header's order
    const double alpha = delta - a.shift;
    const double betan = sqrt(yy);
    const double oldeps = st.eps;
    const double t1 = st.cs * st.dbar, t2 = st.sn * alpha; const double dl = t1 + t2;
    const double t3 = st.sn * st.dbar, t4 = st.cs * alpha; const double gbar = t3 - t4;
    const double eps = st.sn * betan;
    const double cb = st.cs * betan; const double dbar = -cb;
    const double g2 = gbar * gbar, b2 = betan * betan; const double gamma = sqrt(g2 + b2);
    const double ig = 1.0 / gamma;
    const double cs = gbar * ig, sn = betan * ig;
    const double phi = cs * st.phibar, phibar = sn * st.phibar;
    if (!finite_value(gamma) || !finite_value(ig) || !finite_value(phi) || gamma == 0.0) {      // breakdown: before this body's updates
        if (publisher) {
            StopDecision d;
            const double rrOld = st.phibar * st.phibar;
            d.res = fabs(st.phibar); d.shown = a.f.rule == MGCG_RULE_VIENNACL ? sqrt(rrOld / rr0) : d.res; d.stop = true; d.status = MGCG_NONFINITE;
            publish_iteration<0>(a.f, d, k + 1, rrOld, 0.0, 0, [] {});
        }
        return;
    }
    const double rr = phibar * phibar;
    StopDecision d = decide_stop(a.f, rr, 0.0, rr0, k + 1);
    const bool exhausted = betan == 0.0;                // the Krylov space is exhausted: the loop ends with this body
    if (exhausted && !d.stop) { d.stop = true; d.status = MGCG_OK; }
    if (publisher) {
        MinresScalars::State& o = a.ms->st[(k + 1) & 1];
        o.beta = betan; o.cs = cs; o.sn = sn; o.dbar = dbar; o.eps = eps; o.phibar = phibar;
        a.f.sc->alpha = alpha; a.f.sc->beta = betan;
        publish_iteration<0>(a.f, d, k + 1, rr, 0.0, 0, [] {});
    }

    const bool hasW1 = k >= 2, hasW2 = k >= 1;
    const double ib = exhausted ? 0.0 : 1.0 / betan;
    struct Elem { double y, v, w1, w2, x; };
    // one element; e.w1 leaves as w, e.y as vnext (as y when the space is exhausted)
    auto step = [&](Elem& e) {
        double w = e.v;
        if (hasW1) { double t = oldeps * e.w1; w = w - t; }
        if (hasW2) { double t = dl * e.w2; w = w - t; }
        w = w * ig;
        double pw = phi * w; e.x = e.x + pw;
        e.w1 = w;
        if (!exhausted) e.y = e.y * ib;
    };
    auto one = [&](long long i) {
        Elem e = { a.y[i], a.v[i], hasW1 ? a.w1[i] : 0.0, hasW2 ? a.w2[i] : 0.0, a.x[i] };
        step(e);
        a.y[i] = e.y; a.w1[i] = e.w1; a.x[i] = e.x;
    };
    d2* y2 = (d2*)a.y; d2* w12 = (d2*)a.w1; d2* x2 = (d2*)a.x;
    const d2* v2 = (const d2*)a.v; const d2* w22 = (const d2*)a.w2;
    struct Pair { d2 y, v, w1, w2, x; };
    auto load = [&](Pair& p, long long i) {
        p.w1 = {}; p.w2 = {};
        p.y = ldv<NTV>(y2 + i); p.v = ldv<NTV>(v2 + i); p.x = ldv<NTV>(x2 + i);
        if (hasW1) p.w1 = ldv<NTV>(w12 + i);
        if (hasW2) p.w2 = ldv<NTV>(w22 + i);
    };
    auto finish = [&](const Pair& p, long long i) {
        Elem e0 = { p.y.x, p.v.x, p.w1.x, p.w2.x, p.x.x }, e1 = { p.y.y, p.v.y, p.w1.y, p.w2.y, p.x.y };
        step(e0); step(e1);
        d2 o;
        o.x = e0.y; o.y = e1.y; stv<NTV>(o, y2 + i);
        o.x = e0.w1; o.y = e1.w1; stv<NTV>(o, w12 + i);
        o.x = e0.x; o.y = e1.x; stv<NTV>(o, x2 + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// The start and the closing pass: r = t + shift x (t = b - A x from the product's EPI_RESIDUAL epilogue), the product rounded first, and the
// partial sums of r.r.  Twice per call, so the plain element-wise form.
__global__ __launch_bounds__(kBlock) void minres_residual_kernel(const double* __restrict__ t, const double* __restrict__ x, double* __restrict__ r,
                                                                 long long n, double shift, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { double sx = shift * x[i]; double ri = t[i] + sx; r[i] = ri; double q = ri * ri; acc += q; });
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The scalars in front of body 0 (one workgroup).  !reduceFirst (several ranks): r0.r0 is all-reduced already, in red[1].
__global__ __launch_bounds__(kBlock) void minres_init_kernel(const double* __restrict__ partials, int n, int reduceFirst, FinalizeArgs f, MinresScalars* ms)
{
    __shared__ double s_red[4];
    double rr0 = 0.0;
    if (reduceFirst) rr0 = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    if (!reduceFirst) rr0 = ms->red[1];
    const double beta1 = sqrt(rr0);
    publish_start(f, rr0, beta1);
    ms->fDone = 0;
    MinresScalars::State& o = ms->st[0];
    o.beta = 0.0; o.cs = -1.0; o.sn = 0.0; o.dbar = 0.0; o.eps = 0.0; o.phibar = beta1;
    if (!positive_finite(rr0)) refuse_start(f);        // nothing to normalise: b - (A - shift I) x is zero or not finite
}

// v = r * (1 / beta1), in place
__global__ __launch_bounds__(kBlock) void minres_scale_kernel(double* __restrict__ v, long long n, const CgScalars* sc, const MinresScalars* ms)
{
    if (sc->done != 0) return;
    const double inv = 1.0 / ms->st[0].phibar;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { v[i] = v[i] * inv; });
}

int minres_enqueue_residual(Workspace* ws, const double* t, const double* x, double* r, long long n, double shift)
{
    hipStream_t s = ws->stream;
    double* partials = minres_yy_partials(ws);
    const int grid = grid_for(n, 2);
    hipLaunchKernelGGL(minres_residual_kernel, dim3(grid), dim3(kBlock), 0, s, t, x, r, n < 0 ? 0 : n, shift, partials);
    if (dot_reference_order()) { launch_dot_serial(s, r, r, n, partials, nullptr); return 1; }   // the sum in the reference's order replaces the partial sums
    return grid;
}

void minres_enqueue_start(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst, double* v, long long n)
{
    hipStream_t s = ws->stream;
    hipLaunchKernelGGL(minres_init_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)minres_yy_partials(ws), nPartials, reduceFirst ? 1 : 0, f, ws->minresScalars);
    if (n > 0) hipLaunchKernelGGL(minres_scale_kernel, dim3(grid_for(n, 2)), dim3(kBlock), 0, s, v, n, (const CgScalars*)ws->scalars, (const MinresScalars*)ws->minresScalars);
}

static MinresPass minres_pass_args(const MinresRun& R, int k)
{
    MinresPass a{};
    a.ms = R.ws->minresScalars; a.k = k; a.shift = R.shift;
    a.x = R.x; a.y = R.vprev; a.w1 = R.w1; a.q = R.q; a.v = R.v; a.w2 = R.w2; a.n = R.n;
    return a;
}

int minres_enqueue_lanczos(const MinresRun& R, int k, int nDelta)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    MinresPass a = minres_pass_args(R, k);
    a.f.sc = ws->scalars;
    a.inPartials = ws->partials; a.nIn = nDelta; a.outPartials = minres_yy_partials(ws);
    const bool v2 = al16(a.q) && al16(a.v) && al16(a.y);
    // the grid of update_xp_final_kernel; a rank without rows: one workgroup, for the scalar step
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto GIVEN) {
            hipLaunchKernelGGL((minres_lanczos_kernel<V2.value, NTV.value, GIVEN.value>), dim3(grid), dim3(kBlock), 0, s, a);
        }, R.given);
    });
    if (dot_reference_order()) { launch_dot_serial(s, a.y, a.y, R.n, a.outPartials, &ws->scalars->done); return 1; }   // y.y in the reference's order
    return grid;
}

void minres_enqueue_update(const MinresRun& R, const FinalizeArgs& f, int k, int nYY)
{
    Workspace* ws = R.ws;
    MinresPass a = minres_pass_args(R, k);
    a.f = f;
    a.inPartials = minres_yy_partials(ws); a.nIn = nYY;
    const bool v2 = al16(a.x) && al16(a.y) && al16(a.w1) && al16(a.v) && al16(a.w2);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto GIVEN) {
            hipLaunchKernelGGL((minres_update_kernel<V2.value, NTV.value, GIVEN.value>), dim3(grid), dim3(kBlock), 0, ws->stream, a);
        }, R.given);
    });
}

void preload_kernels_minres() { preload_code_object(reinterpret_cast<const void*>(&minres_init_kernel)); }

} // namespace mgcg
