// LSQR for gfx950 (MgcgSolveLsqr): Paige and Saunders' least-squares method for min || A x - b ||_2 (with damp: + damp^2 || x ||^2), A any CSR
// matrix of rows x columns.  include/MgcgGpu.h has the method and its rounding contract; solver.hip's lsqr_solve the host's side.
//
// The two vectors of the Golub-Kahan bidiagonalisation stay unnormalised in memory: uh = beta u (rows) and vh = alpha v (columns), with alpha
// and beta on the device.  Per body, behind the product q = A vh (launch_spmv_auto on A) and behind t = A^T uh (launch_spmv_auto on A^T):
//     pass U  lsqr_u_kernel   (rows)     uh = q * (1 / alpha) - (alpha / beta) * uh, and the partial sums of uh.uh     (2 reads, 1 write: 24 bytes per row)
//     pass V  lsqr_v_kernel   (columns)  beta' = sqrt(uh.uh), the rotation's half that needs beta' alone (rho, c, s, phi), then in one sweep
//                                        vn = vh * (1 / alpha) ; w = vn - (theta / rho of the body before) * w ; x = x + (phi / rho) * w ;
//                                        vh = t * (1 / beta') - beta' * vn, and the partial sums of vh.vh            (4 reads, 3 writes: 56 bytes per column)
//     scalars lsqr_scalars_kernel (one workgroup)  alpha' = sqrt(vh.vh), theta, rhobar, phibar, g = |phibar| alpha' |c|, the stop decision on
//                                        (g^2, g0^2), the trace entry, the host mirror and the state of the next body
// A body is five launches with two reduction points.  EVERY workgroup of pass V adds pass U's partial sums in one fixed order
// (reduce_partials_block), so all of them compute the same scalars; its first workgroup leaves them in LsqrScalars::rot for the scalar
// launch, which alone writes the state that the passes read -- no pass reads a field that a workgroup of the same launch writes.
//
// The stop flag is CgScalars::done.  Pass U, which raises nothing, copies the flag as it found it into LsqrScalars::fDone, and pass V, which
// raises the live flag itself when the rotation breaks down, looks there.  Launches enqueued behind a raised flag return at their first instruction.
//
// Same grid, chunked 16-byte accesses and streaming hints as the MINRES passes (vec_passes.hpp); the rows pass and the columns pass have
// each their own grid.
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_lsqr()
{
    if (lsqrScalars) return true;
    return MGCG_HIP(hipMalloc((void**)&lsqrScalars, sizeof(LsqrScalars)));
}

// pass U's partial sums of uh.uh (and the start's of b.b, the close's of r.r): the first region of the workspace's buffer -- the products of
// this loop have no sum of their own; pass V's of vh.vh (the start's too, the close's of t.t): the second
double* lsqr_uu_partials(Workspace* ws) { return ws->partials; }
double* lsqr_vv_partials(Workspace* ws) { return ws->partials + kMaxPartials; }
static_assert(kMaxGrid <= kMaxPartials, "a pass has at most kMaxGrid workgroups");

struct LsqrPass {
    FinalizeArgs f;
    LsqrScalars* ls;
    const double* inPartials; int nIn;                // pass V: pass U's partial sums of uh.uh; the scalar launch: pass V's of vh.vh
    double* outPartials;
    int k;                                            // the body's index: the host's count, which is the device's while the loop is live
    double damp;
    double *x, *uh, *vh, *w;
    const double *q, *t;
    long long rows, columns;
};

template <bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void lsqr_u_kernel(LsqrPass a)
{
    __shared__ double s_red[4];
    const int done = a.f.sc->done;                     // nobody writes it while this pass runs
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (publisher) a.ls->fDone = done;
    if (done != 0) return;
    const double alpha = a.ls->alpha, beta = a.ls->beta;
    const double ia = 1.0 / alpha;
    const double ab = alpha / beta;
    double acc = 0.0;
    // one element: every product into a double of its own, then the subtraction
    auto step = [&](double q, double u) {
        double qa = q * ia; double au = ab * u; double un = qa - au;
        double t = un * un; acc += t;
        return un;
    };
    auto one = [&](long long i) { a.uh[i] = step(a.q[i], a.uh[i]); };
    const d2* q2 = (const d2*)a.q; d2* u2 = (d2*)a.uh;
    struct Pair { d2 q, u; };
    auto load = [&](Pair& e, long long i) { e.q = ldv<NTV>(q2 + i); e.u = ldv<NTV>(u2 + i); };
    auto finish = [&](const Pair& e, long long i) { d2 o; o.x = step(e.q.x, e.u.x); o.y = step(e.q.y, e.u.y); stv<NTV>(o, u2 + i); };
    stream_pairs<V2, Pair>(a.rows, publisher, load, finish, one);
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0) a.outPartials[blockIdx.x] = t;
}

template <bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void lsqr_v_kernel(LsqrPass a)
{
    __shared__ double s_red[4], s_red2[4];
    if (a.ls->fDone != 0) return;                      // the flag as pass U found it: this pass raises the live one itself
    const double uu = reduce_partials_block(a.inPartials, a.nIn, s_red, 0);
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const bool first = a.k == 0;
    const double alpha = a.ls->alpha, tr = a.ls->tr, phibarOld = a.ls->phibar, rhobarOld = a.ls->rhobar;
    double psi2 = a.ls->psi2;
    // the half of the rotation that needs beta' alone, every product rounded before the add that follows it, in the header's order
    const double betan = sqrt(uu);
    double rhobar = rhobarOld, phibar = phibarOld;
    if (a.damp != 0.0) {
        const double r2 = rhobarOld * rhobarOld, l2 = a.damp * a.damp; const double rd = sqrt(r2 + l2);
        const double lr = a.damp / rd; const double psi = lr * phibarOld;
        const double cr = rhobarOld / rd; phibar = cr * phibarOld;
        const double pp = psi * psi; psi2 = psi2 + pp;
        rhobar = rd;
    }
    const double r2 = rhobar * rhobar, b2 = betan * betan; const double rho = sqrt(r2 + b2);
    const double c = rhobar / rho, s = betan / rho;
    const double phi = c * phibar, phibarn = s * phibar;
    const double xs = phi / rho;
    if (!finite_value(betan) || !finite_value(rho) || rho == 0.0 || !finite_value(xs) || !finite_value(phibarn) || !finite_value(psi2)) {   // breakdown: before this body's updates
        if (publisher) publish_breakdown(a.f, a.k + 1);
        return;
    }
    const bool exhausted = betan == 0.0;                // u is exhausted: g = 0 with this body's x; vh is not formed
    if (publisher) {
        LsqrScalars::Rotation& o = a.ls->rot;
        o.betan = betan; o.rho = rho; o.c = c; o.s = s; o.phibarn = phibarn; o.psi2 = psi2;
    }
    const double ia = 1.0 / alpha;
    const double ib = exhausted ? 0.0 : 1.0 / betan;
    double acc = 0.0;
    struct Elem { double v, w, x, t; };
    // one element; e.v leaves as the next vh (as it came when u is exhausted)
    auto step = [&](Elem& e) {
        const double vn = e.v * ia;
        double w = vn;
        if (!first) { double tw = tr * e.w; w = vn - tw; }
        double pw = xs * w; e.x = e.x + pw;
        e.w = w;
        if (!exhausted) { double tb = e.t * ib; double bv = betan * vn; e.v = tb - bv; double vv = e.v * e.v; acc += vv; }
    };
    auto one = [&](long long i) {
        Elem e = { a.vh[i], first ? 0.0 : a.w[i], a.x[i], a.t[i] };
        step(e);
        a.vh[i] = e.v; a.w[i] = e.w; a.x[i] = e.x;
    };
    d2* v2 = (d2*)a.vh; d2* w2 = (d2*)a.w; d2* x2 = (d2*)a.x; const d2* t2 = (const d2*)a.t;
    struct Pair { d2 v, w, x, t; };
    auto load = [&](Pair& p, long long i) {
        p.w = {};
        p.v = ldv<NTV>(v2 + i); p.x = ldv<NTV>(x2 + i); p.t = ldv<NTV>(t2 + i);
        if (!first) p.w = ldv<NTV>(w2 + i);
    };
    auto finish = [&](const Pair& p, long long i) {
        Elem e0 = { p.v.x, p.w.x, p.x.x, p.t.x }, e1 = { p.v.y, p.w.y, p.x.y, p.t.y };
        step(e0); step(e1);
        d2 o;
        o.x = e0.v; o.y = e1.v; stv<NTV>(o, v2 + i);
        o.x = e0.w; o.y = e1.w; stv<NTV>(o, w2 + i);
        o.x = e0.x; o.y = e1.x; stv<NTV>(o, x2 + i);
    };
    stream_pairs<V2, Pair>(a.columns, publisher, load, finish, one);
    const double t = block_sum(acc, s_red2);
    if (threadIdx.x == 0) a.outPartials[blockIdx.x] = t;
}

// The scalar step behind pass V (one workgroup): alpha' and what follows from it, the stop decision, the state of the next body.
__global__ __launch_bounds__(kBlock) void lsqr_scalars_kernel(LsqrPass a)
{
    __shared__ double s_red[4];
    if (a.f.sc->done != 0) return;                     // one workgroup: nobody else raises it while this launch runs
    const double vv = reduce_partials_block(a.inPartials, a.nIn, s_red, 0);
    if (threadIdx.x != 0) return;
    LsqrScalars* ls = a.ls;
    const LsqrScalars::Rotation o = ls->rot;
    const double alphan = o.betan == 0.0 ? 0.0 : sqrt(vv);
    const double theta = o.s * alphan;
    const double ca = o.c * alphan; const double rhobarn = -ca;
    const double tr = theta / o.rho;
    const double pa = fabs(o.phibarn) * alphan; const double g = pa * fabs(o.c);
    const double gg = g * g;
    const double p2 = o.phibarn * o.phibarn; const double resNorm = sqrt(p2 + o.psi2);
    StopDecision d = decide_stop(a.f, gg, 0.0, a.f.sc->rr0, a.k + 1);
    if (g == 0.0) { d.stop = true; d.status = MGCG_OK; }   // beta' or alpha' exactly zero: x solves the problem, whatever the rule says
    ls->resNorm = resNorm;
    publish_iteration<0>(a.f, d, a.k + 1, gg, 0.0, 0, [&] {
        ls->alpha = alphan; ls->beta = o.betan; ls->phibar = o.phibarn; ls->rhobar = rhobarn; ls->psi2 = o.psi2; ls->tr = tr;
    });
}

// The start, first half (one workgroup): beta1 = sqrt(b.b) from the partial sums of b.b
__global__ __launch_bounds__(kBlock) void lsqr_init_beta_kernel(const double* __restrict__ partials, int n, LsqrScalars* ls)
{
    __shared__ double s_red[4];
    const double bb = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    ls->bb = bb; ls->beta = sqrt(bb);
}

// vh = t * (1 / beta1) with t = A^T b, and the partial sums of vh.vh.  Once per call, so the plain element-wise form.
__global__ __launch_bounds__(kBlock) void lsqr_start_v_kernel(const double* __restrict__ t, double* __restrict__ vh, long long n, const LsqrScalars* ls,
                                                              double* __restrict__ partials)
{
    __shared__ double s_red[4];
    const double ib = 1.0 / ls->beta;
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) { double v = t[i] * ib; vh[i] = v; double q = v * v; acc += q; });
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The start, second half (one workgroup): alpha1, g0 = alpha1 beta1, the scalars in front of body 0.  note: which of the two was zero or
// not finite (1: beta1 -- alpha1 is then not looked at and g0 := beta1; 2: alpha1; 3: neither, but g0^2 is).
__global__ __launch_bounds__(kBlock) void lsqr_init_kernel(const double* __restrict__ partials, int n, FinalizeArgs f, LsqrScalars* ls)
{
    __shared__ double s_red[4];
    const double vv = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    const double bb = ls->bb, beta1 = ls->beta;
    const double alpha1 = sqrt(vv);
    double g0 = alpha1 * beta1; double gg0 = g0 * g0;
    int note = 0;
    if (!positive_finite(bb)) { note = 1; g0 = beta1; gg0 = bb; }
    else if (!positive_finite(vv)) note = 2;
    else if (!positive_finite(gg0)) note = 3;
    publish_start(f, gg0, g0);
    ls->fDone = 0; ls->note = note;
    ls->alpha = alpha1; ls->phibar = beta1; ls->rhobar = alpha1; ls->psi2 = 0.0; ls->tr = 0.0; ls->resNorm = beta1;
    ls->red[0] = 0.0; ls->red[1] = 0.0;
    if (note != 0) refuse_start(f);                    // nothing to normalise
}

// The close: t = t - (damp * damp) * x (damp != 0 only), the product rounded first, and the partial sums of t.t
__global__ __launch_bounds__(kBlock) void lsqr_normal_residual_kernel(double* __restrict__ t, const double* __restrict__ x, long long n, double damp,
                                                                      double* __restrict__ partials)
{
    __shared__ double s_red[4];
    const double l2 = damp * damp;
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        double ti = t[i];
        if (damp != 0.0) { double lx = l2 * x[i]; ti = ti - lx; t[i] = ti; }
        double q = ti * ti; acc += q;
    });
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// the partial sums of v.v into `partials` (1 under dot_order = 1: the sum in the reference's order); returns their number
static int lsqr_enqueue_sumsq(hipStream_t s, const double* v, long long n, double* partials, const int* done)
{
    if (dot_reference_order()) { launch_dot_serial(s, v, v, n, partials, done); return 1; }
    return launch_dot_partials(s, v, v, n, partials);
}

void lsqr_enqueue_start_beta(const LsqrRun& R)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    launch_fill(s, R.x, 0.0, R.columns);                                                 // x = 0 under every rule
    launch_copy(s, R.uh, R.b, R.rows);                                                   // uh = b - A 0
    const int n = lsqr_enqueue_sumsq(s, R.uh, R.rows, lsqr_uu_partials(ws), nullptr);
    hipLaunchKernelGGL(lsqr_init_beta_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)lsqr_uu_partials(ws), n, ws->lsqrScalars);
}

void lsqr_enqueue_start_alpha(const LsqrRun& R, const FinalizeArgs& f)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    double* partials = lsqr_vv_partials(ws);
    int grid = grid_for(R.columns, 2);
    hipLaunchKernelGGL(lsqr_start_v_kernel, dim3(grid), dim3(kBlock), 0, s, R.t, R.vh, R.columns, (const LsqrScalars*)ws->lsqrScalars, partials);
    if (dot_reference_order()) { launch_dot_serial(s, R.vh, R.vh, R.columns, partials, nullptr); grid = 1; }
    hipLaunchKernelGGL(lsqr_init_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)partials, grid, f, ws->lsqrScalars);
}

static LsqrPass lsqr_pass_args(const LsqrRun& R, int k)
{
    LsqrPass a{};
    a.ls = R.ws->lsqrScalars; a.k = k; a.damp = R.damp;
    a.x = R.x; a.uh = R.uh; a.vh = R.vh; a.w = R.w; a.q = R.q; a.t = R.t; a.rows = R.rows; a.columns = R.columns;
    return a;
}

int lsqr_enqueue_u(const LsqrRun& R, int k)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    LsqrPass a = lsqr_pass_args(R, k);
    a.f.sc = ws->scalars;
    a.outPartials = lsqr_uu_partials(ws);
    const bool v2 = al16(a.q) && al16(a.uh);
    const int grid = grid_for(R.rows, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.rows), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((lsqr_u_kernel<V2.value, NTV.value>), dim3(grid), dim3(kBlock), 0, s, a);
    });
    if (dot_reference_order()) { launch_dot_serial(s, a.uh, a.uh, R.rows, a.outPartials, &ws->scalars->done); return 1; }   // uh.uh in the reference's order
    return grid;
}

void lsqr_enqueue_v(const LsqrRun& R, const FinalizeArgs& f, int k, int nUU)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    LsqrPass a = lsqr_pass_args(R, k);
    a.f = f;
    a.inPartials = lsqr_uu_partials(ws); a.nIn = nUU; a.outPartials = lsqr_vv_partials(ws);
    const bool v2 = al16(a.x) && al16(a.vh) && al16(a.w) && al16(a.t);
    int grid = grid_for(R.columns, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.columns), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((lsqr_v_kernel<V2.value, NTV.value>), dim3(grid), dim3(kBlock), 0, s, a);
    });
    if (dot_reference_order()) { launch_dot_serial(s, a.vh, a.vh, R.columns, a.outPartials, &ws->scalars->done); grid = 1; }   // vh.vh in the reference's order
    a.inPartials = a.outPartials; a.nIn = grid;
    hipLaunchKernelGGL(lsqr_scalars_kernel, dim3(1), dim3(kBlock), 0, s, a);
}

int lsqr_enqueue_close_residual(const LsqrRun& R)
{
    return lsqr_enqueue_sumsq(R.ws->stream, R.uh, R.rows, lsqr_uu_partials(R.ws), nullptr);
}

int lsqr_enqueue_close_normal(const LsqrRun& R)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    double* partials = lsqr_vv_partials(ws);
    const int grid = grid_for(R.columns, 2);
    hipLaunchKernelGGL(lsqr_normal_residual_kernel, dim3(grid), dim3(kBlock), 0, s, R.t, (const double*)R.x, R.columns, R.damp, partials);
    if (dot_reference_order()) { launch_dot_serial(s, R.t, R.t, R.columns, partials, nullptr); return 1; }
    return grid;
}

void preload_kernels_lsqr() { preload_code_object(reinterpret_cast<const void*>(&lsqr_init_kernel)); }

} // namespace mgcg
