// BiCGStab for gfx950 (SolveBicgstab* / SolveBicgstabJacobi* / SolveBicgstabMg): van der Vorst's method for A x = b with A any CSR matrix,
// symmetric or not, right-preconditioned with M = I, M = diag(A) or the V-cycle of a hierarchy, so that r stays the residual of the system
// itself.  include/MgcgGpu.h has the method and its rounding contract; solver.hip's cg_solve_bicgstab the host's side.  Out of scope: the
// V-cycle on several ranks (SolveBicgstabMgParallel), BiCGStab(l), GMRES, residual replacement, the block and mixed combinations, the C++ twin
// under host/.
//
// Per body k two products (launch_spmv_auto with the EPI_DOT epilogue: v = A phat with the partial sums of sigma = rhat.v, t = A shat with those of
// theta = s.t) and four passes -- bytes per row without / with the diagonal:
//     pass S    bicgstab_s_kernel    alpha = rho / sigma ; s = r - alpha v ; shat = dinv s           reads r, v (, dinv), writes s (, shat)        24 / 40
//     tau       bicgstab_tau_kernel  the partial sums of t.t                                          reads t                                        8 /  8
//     pass X    bicgstab_x_kernel    omega = theta / tau ; x = (x + alpha phat) + omega shat ; r = s - omega t ; the partial sums of r.r and rhat.r
//                                                                                                     reads x, phat, shat (, s), t, rhat, writes x, r 56 / 64
//     pass P    bicgstab_p_kernel    the stop decision on r.r ; beta ; p = r + beta (p - omega v) ; phat = dinv p
//                                                                                                     reads r, p, v (, dinv), writes p (, phat)      32 / 48
// 120 bytes per row without the diagonal, 160 with it.  Without the diagonal phat IS p and shat IS s: nothing is multiplied and no hatted copy is
// stored (pass X then reads one vector fewer than the six its general form names).  With it s is written over r -- the two are never alive
// together -- and p lives in a buffer of its own, so that both forms take the same seven work vectors.
// The V-cycle form (HAT_STORED) takes the diagonal form's vectors, but the hatted copies are written between the passes by the hierarchy's cycle
// (p -> phat in front of the first product, s -> shat in front of the second), so pass S and pass P write no hatted copy and read no dinv, and
// pass X takes its general six-vector form: 24 + 8 + 64 + 32 = 128 bytes per row.
// A body is six launches with three reduction points: sigma, {theta, tau}, {rr, rhon}.  The scalars stay on the device (BicgstabScalars): every
// workgroup of a pass adds the partial sums in front of it in one fixed order (reduce_partials_block), so all of them compute the same alpha,
// omega, beta, breakdown tests and stop decision, and the first alone persists them, the trace entry and the host mirror.
// Several ranks (GIVEN): the sums are folded by one small launch per reduction point, all-reduced in place in red[0], red[1 .. 2], red[3 .. 4],
// and the passes take them as given.  A rank without rows launches every pass with one workgroup for the scalar steps.
//
// The stop flag is CgScalars::done, and pass P alone raises it.  Pass S, the first pass of a body, copies the flag as it found it into
// BicgstabScalars::fDone; pass X and pass P look there, never at the live flag, which pass P raises while its other workgroups may still start.
// A pass that meets a breakdown (S: sigma; X: omega) changes no vector in any workgroup -- all of them take the same decision from the same
// sums -- and its first workgroup leaves a note (brokeS, brokeX) that only LATER launches read: pass X returns at brokeS, and pass P publishes
// the breakdown.  So no workgroup ever reads a flag that a workgroup of the same launch writes.
//
// Same grid, chunked 16-byte accesses and streaming hints as update_xp_final_kernel and minres_update_kernel (vec_passes.hpp).
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_bicgstab()
{
    if (bicgstabScalars) return true;
    return MGCG_HIP(hipMalloc((void**)&bicgstabScalars, sizeof(BicgstabScalars)));
}

// The product's epilogue fills the first region of the workspace's buffer (sigma, then theta); t.t takes the second, r.r and rhat.r the two
// halves of the third.
double* bicgstab_tau_partials(Workspace* ws) { return ws->partials + kMaxPartials; }
double* bicgstab_rr_partials(Workspace* ws) { return ws->partials + 2 * kMaxPartials; }
double* bicgstab_rho_partials(Workspace* ws) { return ws->partials + 2 * kMaxPartials + kMaxPartials / 2; }
static_assert(kMaxGrid <= kMaxPartials / 2, "a pass has at most kMaxGrid workgroups");

struct BicgstabPass {
    FinalizeArgs f;
    BicgstabScalars* bs;
    const double *inA, *inB; int nA, nB;              // the partial sums in front of the pass (one rank): S sigma; X theta, tau; P r.r, rhat.r
    double *outA, *outB;                              // pass X: r.r, rhat.r
    int k;                                            // the body's index: the host's count, which is the device's while the loop is live
    double *x, *r, *p, *s, *phat, *shat;              // s may be r (with dinv); phat may be p and shat may be s (without): no __restrict__ here
    const double *v, *t, *rhat, *dinv;
    long long n;
};

// HAT (vec_passes.hpp), one template parameter of every pass and of the start: who forms the hatted copies phat = M^-1 p and shat = M^-1 s --
// nobody (phat IS p, shat IS s), the passes themselves, or the V-cycle between the passes.

template <bool V2, bool NTV, bool GIVEN, int HAT>
__global__ __launch_bounds__(kBlock) void bicgstab_s_kernel(BicgstabPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;             // the hatted copy is formed here; HAT_STORED: the cycle writes it behind this pass
    __shared__ double s_red[4];
    const int done = a.f.sc->done;                     // nobody writes it while this pass runs
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (publisher) { a.bs->fDone = done; a.bs->brokeS = 0; a.bs->brokeX = 0; }
    if (done != 0) return;
    double sigma;
    if constexpr (GIVEN) sigma = a.bs->red[0];
    else sigma = reduce_partials_block(a.inA, a.nA, s_red, 0);
    const double rho = a.bs->rho[a.k & 1];
    const double alpha = rho / sigma;
    if (sigma == 0.0 || !finite_value(sigma) || !finite_value(alpha)) {
        if (publisher) a.bs->brokeS = 1;
        return;
    }
    if (publisher) { a.bs->alpha = alpha; a.f.sc->alpha = alpha; }
    // one element: the product into a double of its own, then the subtraction
    auto step = [&](double r, double v) { double av = alpha * v; return r - av; };
    auto one = [&](long long i) {
        const double s = step(a.r[i], a.v[i]);
        a.s[i] = s;
        if constexpr (DINV) a.shat[i] = a.dinv[i] * s;
    };
    const d2* r2 = (const d2*)a.r; const d2* v2 = (const d2*)a.v; const d2* d2p = (const d2*)a.dinv;
    d2* s2 = (d2*)a.s; d2* h2 = (d2*)a.shat;
    struct Pair { d2 r, v, d; };
    auto load = [&](Pair& e, long long i) { e.d = {}; e.r = ldv<NTV>(r2 + i); e.v = ldv<NTV>(v2 + i); if constexpr (DINV) e.d = ldv<NTV>(d2p + i); };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = step(e.r.x, e.v.x); o.y = step(e.r.y, e.v.y);
        stv<NTV>(o, s2 + i);
        if constexpr (DINV) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, h2 + i); }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// the partial sums of t.t: one read per element
template <bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void bicgstab_tau_kernel(const double* __restrict__ t, long long n, double* __restrict__ partials, const int* done)
{
    __shared__ double s_red[4];
    if (*done != 0) return;
    double acc = 0.0;
    grid_stride<V2>(n,
        [&](long long i) { const d2 tv = ldv<NTV>((const d2*)(t + i)); double q0 = tv.x * tv.x; double q1 = tv.y * tv.y; acc += q0; acc += q1; },
        [&](long long i) { double q = t[i] * t[i]; acc += q; });
    const double sum = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

template <bool V2, bool NTV, bool GIVEN, int HAT>
__global__ __launch_bounds__(kBlock) void bicgstab_x_kernel(BicgstabPass a)
{
    constexpr bool HATTED = HAT != HAT_NONE;           // shat is a vector of its own, whoever wrote it: the general six-vector form
    __shared__ double s_red[4], s_red2[4];
    if (a.bs->fDone != 0 || a.bs->brokeS != 0) return; // both as pass S left them
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    double theta, tau;
    if constexpr (GIVEN) { theta = a.bs->red[1]; tau = a.bs->red[2]; }
    else { theta = reduce_partials_block(a.inA, a.nA, s_red, 0); tau = reduce_partials_block(a.inB, a.nB, s_red2, 0); }
    const double omega = tau == 0.0 ? 0.0 : theta / tau;
    if (!finite_value(omega)) {
        if (publisher) a.bs->brokeX = 1;
        return;
    }
    const double alpha = a.bs->alpha;
    if (publisher) a.bs->omega = omega;
    __syncthreads();                                   // s_red, s_red2 are used again below
    double accR = 0.0, accH = 0.0;
    struct Elem { double x, r; };
    // one element, every product into a double of its own; without a hatted copy ph is p and sh is s
    auto step = [&](double x, double ph, double sh, double s, double t, double rh) {
        Elem o;
        double ap = alpha * ph; double x1 = x + ap; double os = omega * sh; o.x = x1 + os;
        double ot = omega * t; o.r = s - ot;
        double q = o.r * o.r; accR += q;
        double h = rh * o.r; accH += h;
        return o;
    };
    auto one = [&](long long i) {
        const double s = a.s[i];
        const Elem o = step(a.x[i], a.phat[i], HATTED ? a.shat[i] : s, s, a.t[i], a.rhat[i]);
        a.x[i] = o.x; a.r[i] = o.r;
    };
    d2* x2 = (d2*)a.x; d2* r2 = (d2*)a.r;
    const d2* p2 = (const d2*)a.phat; const d2* h2 = (const d2*)a.shat; const d2* s2 = (const d2*)a.s;
    const d2* t2 = (const d2*)a.t; const d2* g2 = (const d2*)a.rhat;
    struct Pair { d2 x, ph, sh, s, t, rh; };
    auto load = [&](Pair& e, long long i) {
        e.x = ldv<NTV>(x2 + i); e.ph = ldv<NTV>(p2 + i); e.s = ldv<NTV>(s2 + i); e.t = ldv<NTV>(t2 + i); e.rh = ldv<NTV>(g2 + i);
        if constexpr (HATTED) e.sh = ldv<NTV>(h2 + i); else e.sh = e.s;
    };
    auto finish = [&](const Pair& e, long long i) {
        const Elem o0 = step(e.x.x, e.ph.x, e.sh.x, e.s.x, e.t.x, e.rh.x), o1 = step(e.x.y, e.ph.y, e.sh.y, e.s.y, e.t.y, e.rh.y);
        d2 o;
        o.x = o0.x; o.y = o1.x; stv<NTV>(o, x2 + i);
        o.x = o0.r; o.y = o1.r; stv<NTV>(o, r2 + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    const double sr = block_sum(accR, s_red);
    const double sh = block_sum(accH, s_red2);
    if (threadIdx.x == 0) { a.outA[blockIdx.x] = sr; a.outB[blockIdx.x] = sh; }
}

template <bool V2, bool NTV, bool GIVEN, int HAT>
__global__ __launch_bounds__(kBlock) void bicgstab_p_kernel(BicgstabPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;             // as in pass S
    __shared__ double s_red[4], s_red2[4];
    if (a.bs->fDone != 0) return;                      // the flag as pass S found it: this pass raises the live one itself
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (a.bs->brokeS != 0 || a.bs->brokeX != 0) {      // sigma or omega broke down: x is the iterate of the body before
        if (publisher) publish_breakdown(a.f, a.k + 1);
        return;
    }
    double rr, rhon;
    if constexpr (GIVEN) { rr = a.bs->red[3]; rhon = a.bs->red[4]; }
    else { rr = reduce_partials_block(a.inA, a.nA, s_red, 0); rhon = reduce_partials_block(a.inB, a.nB, s_red2, 0); }
    const int k = a.k;
    const double omega = a.bs->omega, alpha = a.bs->alpha, rho = a.bs->rho[k & 1];
    StopDecision d = decide_stop(a.f, rr, 0.0, a.f.sc->rr0, k + 1);
    if (!d.stop && (omega == 0.0 || rhon == 0.0 || !finite_value(rhon))) { d.stop = true; d.status = MGCG_NONFINITE; }   // x IS this body's iterate
    const double q1 = rhon / rho, q2 = alpha / omega;
    const double beta = q1 * q2;
    if (publisher) publish_iteration<0>(a.f, d, k + 1, rr, 0.0, 0, [&] { a.bs->rho[(k + 1) & 1] = rhon; a.f.sc->beta = beta; });
    if (d.stop) return;
    auto step = [&](double r, double p, double v) { double ov = omega * v; double pm = p - ov; double bp = beta * pm; return r + bp; };
    auto one = [&](long long i) {
        const double p = step(a.r[i], a.p[i], a.v[i]);
        a.p[i] = p;
        if constexpr (DINV) a.phat[i] = a.dinv[i] * p;
    };
    const d2* r2 = (const d2*)a.r; const d2* v2 = (const d2*)a.v; const d2* d2p = (const d2*)a.dinv;
    d2* p2 = (d2*)a.p; d2* h2 = (d2*)a.phat;
    struct Pair { d2 r, p, v, d; };
    auto load = [&](Pair& e, long long i) { e.d = {}; e.r = ldv<NTV>(r2 + i); e.p = ldv<NTV>(p2 + i); e.v = ldv<NTV>(v2 + i); if constexpr (DINV) e.d = ldv<NTV>(d2p + i); };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = step(e.r.x, e.p.x, e.v.x); o.y = step(e.r.y, e.p.y, e.v.y);
        stv<NTV>(o, p2 + i);
        if constexpr (DINV) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, h2 + i); }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// The start behind r = b - A x: rhat = r, p = r, phat = dinv * r (HAT_STORED: phat is left to the cycle) and the partial sums of r.r.  Once
// per call, so the plain element-wise form.
template <int HAT>
__global__ __launch_bounds__(kBlock) void bicgstab_start_kernel(const double* r, double* rhat, double* p, double* phat, const double* dinv, long long n, double* partials)
{
    constexpr bool DINV = HAT == HAT_DINV;
    __shared__ double s_red[4];
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        const double ri = r[i];
        rhat[i] = ri; p[i] = ri;
        if constexpr (DINV) phat[i] = dinv[i] * ri;
        double q = ri * ri; acc += q;
    });
    const double sum = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// The scalars in front of body 0 (one workgroup).  !reduceFirst (several ranks): r0.r0 is all-reduced already, in red[3].
__global__ __launch_bounds__(kBlock) void bicgstab_init_kernel(const double* __restrict__ partials, int n, int reduceFirst, FinalizeArgs f, BicgstabScalars* bs)
{
    __shared__ double s_red[4];
    double rr0 = 0.0;
    if (reduceFirst) rr0 = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    if (!reduceFirst) rr0 = bs->red[3];
    publish_start(f, rr0, sqrt(rr0));
    bs->fDone = 0; bs->brokeS = 0; bs->brokeX = 0; bs->alpha = 0.0; bs->omega = 0.0; bs->rho[0] = rr0; bs->rho[1] = 0.0;
    if (!positive_finite(rr0)) refuse_start(f);        // b - A x is zero or not finite
}

int bicgstab_enqueue_start(const BicgstabRun& R)
{
    hipStream_t s = R.ws->stream;
    double* partials = bicgstab_rr_partials(R.ws);
    const int grid = grid_for(R.n, 2);
    const long long n = R.n < 0 ? 0 : R.n;
    with_hat(R.dinv, R.stored, [&](auto HAT) {
        hipLaunchKernelGGL((bicgstab_start_kernel<HAT.value>), dim3(grid), dim3(kBlock), 0, s, (const double*)R.r, R.rhat, R.p, R.phat, R.dinv, n, partials);
    });
    if (dot_reference_order()) { launch_dot_serial(s, R.r, R.r, n, partials, nullptr); return 1; }   // the sum in the reference's order replaces the partial sums
    return grid;
}

void bicgstab_enqueue_init(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst)
{
    hipLaunchKernelGGL(bicgstab_init_kernel, dim3(1), dim3(kBlock), 0, ws->stream, (const double*)bicgstab_rr_partials(ws), nPartials, reduceFirst ? 1 : 0, f, ws->bicgstabScalars);
}

static BicgstabPass bicgstab_pass_args(const BicgstabRun& R, const FinalizeArgs& f, int k)
{
    BicgstabPass a{};
    a.f = f; a.bs = R.ws->bicgstabScalars; a.k = k;
    a.x = R.x; a.r = R.r; a.p = R.p; a.s = R.s; a.phat = R.phat; a.shat = R.shat; a.v = R.v; a.t = R.t; a.rhat = R.rhat; a.dinv = R.dinv; a.n = R.n;
    return a;
}

// go(V2, NTV, GIVEN, HAT) for the form this call takes
template <typename Go> static void bicgstab_with_form(const BicgstabRun& R, bool v2, Go go)
{
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto GIVEN) { with_hat(R.dinv, R.stored, [&](auto HAT) { go(V2, NTV, GIVEN, HAT); }); }, R.given);
    });
}

void bicgstab_enqueue_s(const BicgstabRun& R, const FinalizeArgs& f, int k, int nSigma)
{
    BicgstabPass a = bicgstab_pass_args(R, f, k);
    a.inA = R.ws->partials; a.nA = nSigma;
    const bool v2 = al16(a.r) && al16(a.v) && al16(a.s) && al16(a.shat) && al16(a.dinv);
    // the grid of update_xp_final_kernel; a rank without rows: one workgroup, for the scalar step
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstab_with_form(R, v2, [&](auto V2, auto NTV, auto GIVEN, auto HAT) {
        hipLaunchKernelGGL((bicgstab_s_kernel<V2.value, NTV.value, GIVEN.value, HAT.value>), dim3(grid), dim3(kBlock), 0, R.ws->stream, a);
    });
}

int bicgstab_enqueue_tau(const BicgstabRun& R)
{
    hipStream_t s = R.ws->stream;
    double* partials = bicgstab_tau_partials(R.ws);
    const int* done = &R.ws->scalars->done;
    const long long n = R.n < 0 ? 0 : R.n;
    if (dot_reference_order()) { launch_dot_serial(s, R.t, R.t, n, partials, done); return 1; }
    const bool v2 = al16(R.t);
    const int grid = grid_for(n, v2 ? 4 : 2);
    with_v2_nt(v2, vec_nt(n), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((bicgstab_tau_kernel<V2.value, NTV.value>), dim3(grid), dim3(kBlock), 0, s, (const double*)R.t, n, partials, done);
    });
    return grid;
}

int bicgstab_enqueue_x(const BicgstabRun& R, const FinalizeArgs& f, int k, int nTheta, int nTau)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    BicgstabPass a = bicgstab_pass_args(R, f, k);
    a.inA = ws->partials; a.nA = nTheta; a.inB = bicgstab_tau_partials(ws); a.nB = nTau;
    a.outA = bicgstab_rr_partials(ws); a.outB = bicgstab_rho_partials(ws);
    const bool v2 = al16(a.x) && al16(a.r) && al16(a.phat) && al16(a.shat) && al16(a.s) && al16(a.t) && al16(a.rhat);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstab_with_form(R, v2, [&](auto V2, auto NTV, auto GIVEN, auto HAT) {
        hipLaunchKernelGGL((bicgstab_x_kernel<V2.value, NTV.value, GIVEN.value, HAT.value>), dim3(grid), dim3(kBlock), 0, s, a);
    });
    if (dot_reference_order()) {                       // r.r and rhat.r in the reference's order
        const int* done = &ws->scalars->done;
        const long long n = R.n < 0 ? 0 : R.n;
        launch_dot_serial(s, a.r, a.r, n, a.outA, done);
        launch_dot_serial(s, a.rhat, a.r, n, a.outB, done);
        return 1;
    }
    return grid;
}

void bicgstab_enqueue_p(const BicgstabRun& R, const FinalizeArgs& f, int k, int nRr)
{
    Workspace* ws = R.ws;
    BicgstabPass a = bicgstab_pass_args(R, f, k);
    a.inA = bicgstab_rr_partials(ws); a.nA = nRr; a.inB = bicgstab_rho_partials(ws); a.nB = nRr;
    const bool v2 = al16(a.r) && al16(a.p) && al16(a.v) && al16(a.phat) && al16(a.dinv);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstab_with_form(R, v2, [&](auto V2, auto NTV, auto GIVEN, auto HAT) {
        hipLaunchKernelGGL((bicgstab_p_kernel<V2.value, NTV.value, GIVEN.value, HAT.value>), dim3(grid), dim3(kBlock), 0, ws->stream, a);
    });
}

void preload_kernels_bicgstab() { preload_code_object(reinterpret_cast<const void*>(&bicgstab_init_kernel)); }

} // namespace mgcg
