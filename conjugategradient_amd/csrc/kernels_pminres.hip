// Preconditioned MINRES for gfx950 (SolveMinresJacobi / SolveMinresJacobiParallel / SolveMinresMg): Paige and Saunders' method for
// (A - shift I) x = b with a symmetric positive definite preconditioner M -- the diagonal (z = dinv * r, formed per element, no z vector) or
// any operator whose result the host leaves in a vector between the two passes (the V-cycle).  include/MgcgGpu.h has the method and its
// rounding contract; solver.hip's cg_solve_pminres the host's side; kernels_minres.hip the plain loop this one is shaped after.
//
// Per body k, behind the product q = A v (launch_spmv_auto with the EPI_DOT epilogue: the partial sums of v.q), two passes:
//     pass A  pminres_lanczos_kernel  alpha = v.q - shift v.v ; rn = ((q - shift v) - (beta/oldb) r1) - (alpha/beta) r2, in place over r1, and --
//                                     Jacobi -- the partial sums of rn.z, z = dinv rn                  (5 reads, 1 write: 48 bytes per row; 40 with shift == 0)
//     pass B  pminres_update_kernel   the Givens rotation from (alpha, sqrt(rn.z)) and the state of the body before, the stop decision on |phibar|, then
//                                     w = ((v - oldeps w1) - dl w2) / gamma over w1, x = x + phi w, v = z / betan IN PLACE, and the partial sums of the
//                                     new v.v                                                          (6 reads, 3 writes: 72 bytes per row; z given: 5 reads)
// With a z vector (the V-cycle) the host enqueues the operator rn -> z and one dot launch for rn.z between the passes.
// The three regions of the workspace's partial sums hold v.q (the product's epilogue), rn.z (pass A or the dot launch) and v.v (pass B).
// One rank: EVERY workgroup of a pass adds the incoming partial sums in one fixed order (reduce_partials_block), so all of them compute the
// same scalars and take the same stop decision; the first alone persists them (MinresScalars::red, st[(k + 1) & 1]), the trace entry and the
// host mirror.  Several ranks (GIVEN): {v.q, v.v} are folded by one small launch into red[0 .. 1] and all-reduced as one pair, rn.z into
// red[3] the same way; a rank without rows launches both passes with one workgroup for the scalar steps.
//
// The stop flag is handled as in kernels_minres.hip: pass A copies CgScalars::done as it found it into MinresScalars::fDone, and pass B,
// which raises the live flag while its other workgroups may still start, looks there.
#include "vec_passes.hpp"

namespace mgcg {

double* pminres_rz_partials(Workspace* ws) { return ws->partials + kMaxPartials; }
double* pminres_vv_partials(Workspace* ws) { return ws->partials + 2 * kMaxPartials; }

struct PminresPass {
    FinalizeArgs f;
    MinresScalars* ms;
    const double* inA; int nA;                        // pass A: the product's partial sums of v.q; pass B: those of rn.z (one rank)
    const double* inB; int nB;                        // pass A: the partial sums of v.v (one rank)
    double* outPartials;                              // pass A: rn.z (Jacobi); pass B: the new v.v
    int k;                                            // the body's index: the host's count, which is the device's while the loop is live
    double shift;
    double *x, *v, *r1, *w1;                          // r1: pass A writes rn there, pass B (Jacobi) reads it; w1: pass B writes w there; v: in place
    const double *q, *r2, *w2, *dinv, *z;
    long long n;
};

template <bool V2, bool NTV, bool GIVEN, bool JACOBI, bool SHIFTED>
__global__ __launch_bounds__(kBlock) void pminres_lanczos_kernel(PminresPass a)
{
    __shared__ double s_red[4], s_red2[4], s_red3[4];
    const int done = a.f.sc->done;                     // nobody writes it while this pass runs
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (publisher) a.ms->fDone = done;
    if (done != 0) return;
    double vq, vv;
    if constexpr (GIVEN) { vq = a.ms->red[0]; vv = a.ms->red[1]; }
    else {
        vq = reduce_partials_block(a.inA, a.nA, s_red, 0);
        vv = reduce_partials_block(a.inB, a.nB, s_red2, 0);
        if (publisher) { a.ms->red[0] = vq; a.ms->red[1] = vv; }
    }
    const bool first = a.k == 0;
    const MinresScalars::State st = a.ms->st[a.k & 1];
    const double sv = a.shift * vv; const double alpha = vq - sv;
    const double c1 = first ? 0.0 : st.beta / st.oldb;  // the two quotients, once per body
    const double c2 = alpha / st.beta;
    const double shift = a.shift;
    double acc = 0.0;
    // one element: every product into a double of its own, then the subtraction
    auto step = [&](double q, double v, double r1, double r2, double dinv) {
        double y = q;
        if constexpr (SHIFTED) { double t = shift * v; y = q - t; }
        if (!first) { double t = c1 * r1; y = y - t; }
        double t2 = c2 * r2; double rn = y - t2;
        if constexpr (JACOBI) { double z = dinv * rn; double t = rn * z; acc += t; }
        return rn;
    };
    auto one = [&](long long i) {
        a.r1[i] = step(a.q[i], SHIFTED ? a.v[i] : 0.0, first ? 0.0 : a.r1[i], a.r2[i], JACOBI ? a.dinv[i] : 0.0);
    };
    const d2* q2 = (const d2*)a.q; const d2* v2 = (const d2*)a.v; d2* p2 = (d2*)a.r1; const d2* c2v = (const d2*)a.r2; const d2* d2v = (const d2*)a.dinv;
    struct Pair { d2 q, v, p, c, d; };
    auto load = [&](Pair& e, long long i) {
        e.v = {}; e.p = {}; e.d = {};
        e.q = ldv<NTV>(q2 + i); e.c = ldv<NTV>(c2v + i);
        if constexpr (SHIFTED) e.v = ldv<NTV>(v2 + i);
        if (!first) e.p = ldv<NTV>(p2 + i);
        if constexpr (JACOBI) e.d = ldv<NTV>(d2v + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = step(e.q.x, e.v.x, e.p.x, e.c.x, e.d.x); o.y = step(e.q.y, e.v.y, e.p.y, e.c.y, e.d.y);
        stv<NTV>(o, p2 + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    if constexpr (JACOBI) {
        const double t = block_sum(acc, s_red3);
        if (threadIdx.x == 0) a.outPartials[blockIdx.x] = t;
    }
}

template <bool V2, bool NTV, bool GIVEN, bool JACOBI>
__global__ __launch_bounds__(kBlock) void pminres_update_kernel(PminresPass a)
{
    __shared__ double s_red[4], s_red2[4];
    if (a.ms->fDone != 0) return;                      // the flag as pass A found it: this pass raises the live one itself
    const double vq = a.ms->red[0], vv = a.ms->red[1];
    double rz;
    if constexpr (GIVEN) rz = a.ms->red[3];
    else rz = reduce_partials_block(a.inA, a.nA, s_red, 0);
    const int k = a.k;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const MinresScalars::State st = a.ms->st[k & 1];
    const double rr0 = a.f.sc->rr0;
    // the loop ends before this body's updates, repeating the last judged residual
    auto refuse = [&] {
        if (publisher) {
            StopDecision d;
            const double rrOld = st.phibar * st.phibar;
            d.res = fabs(st.phibar); d.shown = a.f.rule == MGCG_RULE_VIENNACL ? sqrt(rrOld / rr0) : d.res; d.stop = true; d.status = MGCG_NONFINITE;
            publish_iteration<0>(a.f, d, k + 1, rrOld, 0.0, 0, [] {});
        }
    };
    if (!(rz >= 0.0 && rz <= kFiniteMax)) { refuse(); return; }                   // M is not positive definite on this residual, or a value that is not finite
    // the rotation, every product rounded before the add or subtraction that follows it, in the header's order
    const double sv = a.shift * vv; const double alpha = vq - sv;
    const double betan = sqrt(rz);
    const double oldeps = st.eps;
    const double t1 = st.cs * st.dbar, t2 = st.sn * alpha; const double dl = t1 + t2;
    const double t3 = st.sn * st.dbar, t4 = st.cs * alpha; const double gbar = t3 - t4;
    const double eps = st.sn * betan;
    const double cb = st.cs * betan; const double dbar = -cb;
    const double g2 = gbar * gbar, b2 = betan * betan; const double gamma = sqrt(g2 + b2);
    const double ig = 1.0 / gamma;
    const double cs = gbar * ig, sn = betan * ig;
    const double phi = cs * st.phibar, phibar = sn * st.phibar;
    if (!finite_value(gamma) || !finite_value(ig) || !finite_value(phi) || gamma == 0.0) { refuse(); return; }      // breakdown
    const double rr = phibar * phibar;
    StopDecision d = decide_stop(a.f, rr, 0.0, rr0, k + 1);
    const bool exhausted = betan == 0.0;                // the Krylov space is exhausted: the loop ends with this body
    if (exhausted && !d.stop) { d.stop = true; d.status = MGCG_OK; }
    if (publisher) {
        MinresScalars::State& o = a.ms->st[(k + 1) & 1];
        o.beta = betan; o.oldb = st.beta; o.cs = cs; o.sn = sn; o.dbar = dbar; o.eps = eps; o.phibar = phibar;
        a.f.sc->alpha = alpha; a.f.sc->beta = betan;
        publish_iteration<0>(a.f, d, k + 1, rr, 0.0, 0, [] {});
    }

    const bool hasW1 = k >= 2, hasW2 = k >= 1;
    const double ib = exhausted ? 0.0 : 1.0 / betan;
    double acc = 0.0;
    struct Elem { double v, w1, w2, x, z, d; };        // z: rn in the Jacobi form (d = dinv), else M^-1 rn
    // one element; e.w1 leaves as w, e.v as the next v (unchanged when the space is exhausted)
    auto step = [&](Elem& e) {
        double w = e.v;
        if (hasW1) { double t = oldeps * e.w1; w = w - t; }
        if (hasW2) { double t = dl * e.w2; w = w - t; }
        w = w * ig;
        double pw = phi * w; e.x = e.x + pw;
        e.w1 = w;
        if (!exhausted) {
            double z = e.z;
            if constexpr (JACOBI) z = e.d * e.z;
            double vn = z * ib; double t = vn * vn; acc += t;
            e.v = vn;
        }
    };
    const double* zin = JACOBI ? a.r1 : a.z;
    auto one = [&](long long i) {
        Elem e = { a.v[i], hasW1 ? a.w1[i] : 0.0, hasW2 ? a.w2[i] : 0.0, a.x[i], zin[i], JACOBI ? a.dinv[i] : 0.0 };
        step(e);
        a.v[i] = e.v; a.w1[i] = e.w1; a.x[i] = e.x;
    };
    d2* v2 = (d2*)a.v; d2* w12 = (d2*)a.w1; d2* x2 = (d2*)a.x;
    const d2* w22 = (const d2*)a.w2; const d2* z2 = (const d2*)zin; const d2* d2v = (const d2*)a.dinv;
    struct Pair { d2 v, w1, w2, x, z, d; };
    auto load = [&](Pair& p, long long i) {
        p.w1 = {}; p.w2 = {}; p.d = {};
        p.v = ldv<NTV>(v2 + i); p.x = ldv<NTV>(x2 + i); p.z = ldv<NTV>(z2 + i);
        if constexpr (JACOBI) p.d = ldv<NTV>(d2v + i);
        if (hasW1) p.w1 = ldv<NTV>(w12 + i);
        if (hasW2) p.w2 = ldv<NTV>(w22 + i);
    };
    auto finish = [&](const Pair& p, long long i) {
        Elem e0 = { p.v.x, p.w1.x, p.w2.x, p.x.x, p.z.x, p.d.x }, e1 = { p.v.y, p.w1.y, p.w2.y, p.x.y, p.z.y, p.d.y };
        step(e0); step(e1);
        d2 o;
        o.x = e0.v; o.y = e1.v; stv<NTV>(o, v2 + i);
        o.x = e0.w1; o.y = e1.w1; stv<NTV>(o, w12 + i);
        o.x = e0.x; o.y = e1.x; stv<NTV>(o, x2 + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    const double t = block_sum(acc, s_red2);
    if (threadIdx.x == 0) a.outPartials[blockIdx.x] = t;
}

// The start: r = t + shift x (t = b - A x from the product's EPI_RESIDUAL epilogue), the product rounded first, and -- JACOBI -- the partial
// sums of r.z, z = dinv r.  Once per call, so the plain element-wise form.
template <bool JACOBI>
__global__ __launch_bounds__(kBlock) void pminres_residual_kernel(const double* __restrict__ t, const double* __restrict__ x, double* __restrict__ r,
                                                                  const double* __restrict__ dinv, long long n, double shift, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        double sx = shift * x[i]; double ri = t[i] + sx; r[i] = ri;
        if constexpr (JACOBI) { double z = dinv[i] * ri; double q = ri * z; acc += q; }
    });
    if constexpr (JACOBI) {
        const double s = block_sum(acc, s_red);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// The scalars in front of body 0 (one workgroup).  !reduceFirst (several ranks): the first r.z is all-reduced already, in red[3].
__global__ __launch_bounds__(kBlock) void pminres_init_kernel(const double* __restrict__ partials, int n, int reduceFirst, FinalizeArgs f, MinresScalars* ms)
{
    __shared__ double s_red[4];
    double bz = 0.0;
    if (reduceFirst) bz = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    if (!reduceFirst) bz = ms->red[3];
    const double beta1 = sqrt(bz);
    publish_start(f, bz, beta1);
    ms->fDone = 0;
    ms->red[4] = bz;                                    // for the host's message: a negative figure says that M is not positive definite
    MinresScalars::State& o = ms->st[0];
    o.beta = beta1; o.oldb = 0.0; o.cs = -1.0; o.sn = 0.0; o.dbar = 0.0; o.eps = 0.0; o.phibar = beta1;
    if (!positive_finite(bz)) refuse_start(f);         // nothing to normalise: the residual is zero, M is not positive definite, or a value is not finite
}

// v = z * (1 / beta1), z = dinv r (JACOBI) or the given vector, and the partial sums of v.v
template <bool JACOBI>
__global__ __launch_bounds__(kBlock) void pminres_scale_kernel(double* __restrict__ v, const double* __restrict__ r, const double* __restrict__ dinv,
                                                               long long n, const CgScalars* sc, const MinresScalars* ms, double* __restrict__ partials)
{
    __shared__ double s_red[4];
    if (sc->done != 0) return;
    const double inv = 1.0 / ms->st[0].phibar;
    double acc = 0.0;
    grid_stride<false>(n, [&](long long) {}, [&](long long i) {
        double z = r[i];
        if constexpr (JACOBI) z = dinv[i] * z;
        double vi = z * inv; v[i] = vi;
        double t = vi * vi; acc += t;
    });
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

int pminres_enqueue_residual(Workspace* ws, const double* t, const double* x, double* r, const double* dinv, long long n, double shift)
{
    hipStream_t s = ws->stream;
    double* partials = pminres_rz_partials(ws);
    const int grid = grid_for(n, 2);
    if (n < 0) n = 0;
    if (!dinv) { hipLaunchKernelGGL(pminres_residual_kernel<false>, dim3(grid), dim3(kBlock), 0, s, t, x, r, dinv, n, shift, partials); return 0; }
    hipLaunchKernelGGL(pminres_residual_kernel<true>, dim3(grid), dim3(kBlock), 0, s, t, x, r, dinv, n, shift, partials);
    if (dot_reference_order()) { launch_dot_serial(s, r, r, n, partials, nullptr, dinv); return 1; }   // the sum in the reference's order replaces the partial sums
    return grid;
}

int pminres_enqueue_start(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst, double* v, const double* r, const double* dinv, const double* z, long long n)
{
    hipStream_t s = ws->stream;
    double* vvPartials = pminres_vv_partials(ws);
    hipLaunchKernelGGL(pminres_init_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)pminres_rz_partials(ws), nPartials, reduceFirst ? 1 : 0, f, ws->minresScalars);
    const int grid = grid_for(n, 2);
    if (n < 0) n = 0;
    // (a rank without rows: one workgroup that writes the one partial sum 0)
    if (dinv) hipLaunchKernelGGL(pminres_scale_kernel<true>, dim3(grid), dim3(kBlock), 0, s, v, r, dinv, n, (const CgScalars*)ws->scalars, (const MinresScalars*)ws->minresScalars, vvPartials);
    else hipLaunchKernelGGL(pminres_scale_kernel<false>, dim3(grid), dim3(kBlock), 0, s, v, z, dinv, n, (const CgScalars*)ws->scalars, (const MinresScalars*)ws->minresScalars, vvPartials);
    if (dot_reference_order()) { launch_dot_serial(s, v, v, n, vvPartials, &ws->scalars->done); return 1; }
    return grid;
}

static PminresPass pminres_pass_args(const PminresRun& R, int k)
{
    PminresPass a{};
    a.ms = R.ws->minresScalars; a.k = k; a.shift = R.shift;
    a.x = R.x; a.v = R.v; a.r1 = R.r1; a.w1 = R.w1; a.q = R.q; a.r2 = R.r2; a.w2 = R.w2; a.dinv = R.dinv; a.z = R.z; a.n = R.n;
    return a;
}

int pminres_enqueue_lanczos(const PminresRun& R, int k, int nVq, int nVv)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    PminresPass a = pminres_pass_args(R, k);
    a.f.sc = ws->scalars;
    a.inA = ws->partials; a.nA = nVq; a.inB = pminres_vv_partials(ws); a.nB = nVv; a.outPartials = pminres_rz_partials(ws);
    const bool jacobi = R.dinv != nullptr;
    const bool v2 = al16(a.q) && al16(a.v) && al16(a.r1) && al16(a.r2) && (!jacobi || al16(a.dinv));
    // the grid of update_xp_final_kernel; a rank without rows: one workgroup, for the scalar step
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto GIVEN, auto JACOBI, auto SHIFTED) {
            hipLaunchKernelGGL((pminres_lanczos_kernel<V2.value, NTV.value, GIVEN.value, JACOBI.value, SHIFTED.value>), dim3(grid), dim3(kBlock), 0, s, a);
        }, R.given, jacobi, R.shift != 0.0);
    });
    if (!jacobi) return 0;
    if (dot_reference_order()) { launch_dot_serial(s, a.r1, a.r1, R.n, a.outPartials, &ws->scalars->done, a.dinv); return 1; }   // rn.z in the reference's order
    return grid;
}

int pminres_enqueue_update(const PminresRun& R, const FinalizeArgs& f, int k, int nRz)
{
    Workspace* ws = R.ws;
    PminresPass a = pminres_pass_args(R, k);
    a.f = f;
    a.inA = pminres_rz_partials(ws); a.nA = nRz; a.outPartials = pminres_vv_partials(ws);
    const bool jacobi = R.dinv != nullptr;
    const bool v2 = al16(a.x) && al16(a.v) && al16(a.w1) && al16(a.w2) && (jacobi ? al16(a.r1) && al16(a.dinv) : al16(a.z));
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_flags([&](auto GIVEN, auto JACOBI) {
            hipLaunchKernelGGL((pminres_update_kernel<V2.value, NTV.value, GIVEN.value, JACOBI.value>), dim3(grid), dim3(kBlock), 0, ws->stream, a);
        }, R.given, jacobi);
    });
    // v.v of the new v in the reference's order.  The flag this launch looks at is the one pass B may just have raised: the loop is over then
    if (dot_reference_order()) { launch_dot_serial(ws->stream, a.v, a.v, R.n, a.outPartials, &ws->scalars->done); return 1; }
    return grid;
}

void preload_kernels_pminres() { preload_code_object(reinterpret_cast<const void*>(&pminres_init_kernel)); }

} // namespace mgcg
