// BiCGStab(l) for gfx950 (SolveBicgstabL / SolveBicgstabLJacobi): Sleijpen and Fokkema's method for A x = b with A any CSR matrix, l = 1 .. 4,
// right-preconditioned with M = I or M = diag(A), one rank.  A body is l BiCG steps, which raise the degree of the residual polynomial by l,
// and ONE minimal-residual step of degree l over r_0 .. r_l, where BiCGStab takes l steps of degree 1: the polynomial may then have complex
// roots, which is what a spectrum near the imaginary axis asks for.  include/MgcgGpu.h has the method and its rounding contract; solver.hip's
// cg_solve_bicgstabl the host's side.  GMRES: kernels_gmres.hip.  Out of scope: several ranks, the V-cycle form, l > 4, residual replacement,
// the C++ twin under host/.
//
// Per body k 2 l products (launch_spmv_auto with the EPI_DOT epilogue and w = rt: u_{j+1} = A hat(u_j) with the partial sums of sigma = rt.u_{j+1},
// r_{j+1} = A hat(r_j) with those of rt.r_{j+1}) and 2 l + 2 passes; vectors read + written, without / with the diagonal (which adds dinv to
// the reads and the gather buffer to the writes of U_j, R_j and P, and dinv to the reads of the combine pass):
//     pass R_j   bicgstabl_r_kernel        alpha = rho / sigma ; r_i -= alpha u_{i+1}, i = 0 .. j ; x += alpha hat(u_0) ; gather = hat(r_j)
//                                                           reads r_0 .. r_j, u_0 .. u_{j+1}, x, writes r_0 .. r_j, x          3 j + 6 / 3 j + 8
//     pass U_j   bicgstabl_u_kernel        (j >= 1) beta = alpha (rho1 / rho) ; u_i = r_i - beta u_i, i = 0 .. j ; gather = hat(u_j)
//                                                           reads r_0 .. r_j, u_0 .. u_j, writes u_0 .. u_j                    3 j + 3 / 3 j + 5
//     Gram       bicgstabl_gram_kernel     the partial sums of Z_ab = r_a.r_b, a = 1 .. l, b = 0 .. a: reads r_0 .. r_l           l + 1 / l + 1
//     combine    bicgstabl_combine_kernel  gamma from Z ; u_0 -= sum gamma_j u_j ; x += sum gamma_j hat(r_{j-1}) ; r_0 -= sum gamma_j r_j ; the partial
//                                          sums of r_0.r_0 and rt.r_0
//                                                           reads u_0 .. u_l, r_0 .. r_l, x, rt, writes u_0, x, r_0             2 l + 7 / 2 l + 8
//     pass P     bicgstabl_p_kernel        the stop decision on r_0.r_0 ; beta ; u_0 = r_0 - beta u_0 ; gather = hat(u_0)
//                                                           reads r_0, u_0, writes u_0                                         3 / 5
// Bytes per row per body -- 8 x [sum over j of (3 j + 6), over j >= 1 of (3 j + 3), (l + 1), (2 l + 7), 3] vectors, and 8 x (4 l + 1) more with the
// diagonal -- and per product:
//     l      vectors   without the diagonal        with it
//     1      20        160    = 80 per product      200   = 100
//     2      38        304    = 76                  376   = 94
//     3      62        496    = 82.7                600   = 100
//     4      92        736    = 92                  872   = 109
// against 120 / 160 per body = 60 / 80 per product in kernels_bicgstab.hip: the passes of a step touch every vector of the steps before it, so the
// traffic grows with l (l + 1) / 2 while the products grow with l.  What the method buys is bodies, not bytes.
// A body is 4 l + 2 launches with 2 l + 2 reduction points: sigma and rho1 per step, Z, {rr, rhon}.  gamma has no launch of its own: every workgroup
// of the combine pass adds the partial sums of the l (l + 3) / 2 entries of Z in front of it and factorises redundantly -- at most 14 fixed-order
// sums of at most kMaxGrid doubles and some two hundred scalar operations per workgroup, against a launch and its drain on the critical path.
// All scalars stay on the device (BicgstablScalars): every workgroup of a pass computes the same alpha, beta, gamma, breakdown tests and stop
// decision from the same sums in the same order (reduce_partials_block), and the first alone persists them, the trace entry and the host mirror.
//
// The stop flag is CgScalars::done, and pass P alone raises it.  Pass R_0, the first pass of a body, copies the flag as it found it into
// BicgstablScalars::fDone and clears broke[0 .. 3]; every later pass of the body looks at the copy, never at the live flag, which pass P raises while
// its other workgroups may still start.  A pass R_j that meets a breakdown changes no vector in any workgroup -- all of them take the same
// decision from the same sums -- and its first workgroup leaves the note broke[j], which only LATER launches read: pass R_j itself looks at
// broke[0 .. j-1], every other pass at all four, and returns; pass P publishes the breakdown.  So no workgroup ever reads a flag that a
// workgroup of the same launch writes.  The products are gated on the live flag and write only u_{j+1} and r_{j+1}, which nothing reads behind
// a breakdown or the stop.
// The stop test is also made in front of steps 1 .. l-1: pass R_j leaves the partial sums of its new r_0.r_0 (no vector is read for them), and
// pass U_{j+1} judges them by the rule in every workgroup; when r_0 meets the test the body ends there -- no vector is changed, the first
// workgroup leaves the note early[j+1], every later pass returns at it and pass P publishes the iteration with that r_0.r_0.  Without it a
// Krylov space that is exhausted inside a body (fewer rows than l, a right-hand side of few eigenvectors) leaves the later steps quotients of
// rounding errors, and alpha of the order 1e15 has been seen to move x by 1e-2 while the recurrence's r_0 stayed at 1e-16.
//
// Same grid, chunked 16-byte accesses and streaming hints as kernels_bicgstab.hip (vec_passes.hpp).
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_bicgstabl()
{
    if (!bicgstablScalars && !MGCG_HIP(hipMalloc((void**)&bicgstablScalars, sizeof(BicgstablScalars)))) return false;
    if (!bicgstablPartials && !MGCG_HIP(hipMalloc((void**)&bicgstablPartials, sizeof(double) * (size_t)(kBicgstablGram + 2) * kMaxGrid))) return false;
    return true;
}

// Region e of the loop's own partial sums: e < kBicgstablGram the entry of Z, then r_0.r_0 and rt.r_0 of the combine pass.
static double* bicgstabl_partials(Workspace* ws, int e) { return ws->bicgstablPartials + (size_t)e * kMaxGrid; }
// Z_ab, a = 1 .. l, b = 0 .. a, lies in region a (a + 1) / 2 - 1 + b
__host__ __device__ constexpr int bicgstabl_entry(int a, int b) { return a * (a + 1) / 2 - 1 + b; }

struct BicgstablPass {
    FinalizeArgs f;
    BicgstablScalars* bs;
    const double* in; int nIn;                         // the partial sums in front of the pass: U rt.r_j; R rt.u_{j+1}; combine Z (regions of kMaxGrid); P r.r
    const double* inB; int nInB;                       // pass P: rt.r_0 (nIn of them too); pass U: r_0.r_0 as pass R_{j-1} left it
    double *outA, *outB;                               // the combine pass: r_0.r_0, rt.r_0; pass R: r_0.r_0
    int k;                                             // the body's index: the host's count, which is the device's while the loop is live
    int ell;
    double *x, *r[kBicgstablMaxL + 1], *u[kBicgstablMaxL + 1], *gather;
    const double *rt, *dinv;
    long long n;
};

// HAT (vec_passes.hpp), one template parameter of every pass: who forms hat(v) = M^-1 v -- nobody (M = I: the products gather from u_j and r_j
// themselves) or the passes (dinv * value per element, stored in the gather buffer for the next product).  HAT_STORED has no form here.
// a pass R_j in front of step `upto` of this body met a breakdown (upto = kBicgstablMaxL: any)
template <int UPTO = kBicgstablMaxL>
__device__ __forceinline__ bool bicgstabl_broke(const BicgstablScalars* bs)
{
    int any = 0;
#pragma unroll
    for (int j = 0; j < UPTO; ++j) any |= bs->broke[j];
    return any != 0;
}
// a pass U_j in front of step `upto` of this body found r_0 converged: the body has ended
template <int UPTO = kBicgstablMaxL>
__device__ __forceinline__ bool bicgstabl_early(const BicgstablScalars* bs)
{
    int any = 0;
#pragma unroll
    for (int j = 0; j < UPTO; ++j) any |= bs->early[j];
    return any != 0;
}

template <bool V2, bool NTV, int HAT, int J>
__global__ __launch_bounds__(kBlock) void bicgstabl_u_kernel(BicgstablPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;
    __shared__ double s_red[4], s_red2[4];
    if (a.bs->fDone != 0 || bicgstabl_broke(a.bs) || bicgstabl_early<J>(a.bs)) return;   // as pass R_0 and the passes behind it left them
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    // r_0 as step J - 1 left it: when it meets the rule's test the body ends here
    const double rr = reduce_partials_block(a.inB, a.nInB, s_red2, 0);
    const StopDecision d = decide_stop(a.f, rr, 0.0, a.f.sc->rr0, a.k + 1);
    if (d.stop && d.status == MGCG_OK) {
        if (publisher) { a.bs->early[J] = 1; a.bs->rrEarly = rr; }
        return;
    }
    const double rho1 = reduce_partials_block(a.in, a.nIn, s_red, 0);
    const double rho = a.bs->rho[a.k & 1][J - 1];
    const double alpha = a.bs->alpha;
    const double ratio = rho1 / rho;
    const double beta = alpha * ratio;
    if (publisher) { a.bs->rho[a.k & 1][J] = rho1; a.f.sc->beta = beta; }
    // one element: the product into a double of its own, then the subtraction
    auto step = [&](double r, double u) { double bu = beta * u; return r - bu; };
    auto one = [&](long long i) {
#pragma unroll
        for (int q = 0; q <= J; ++q) {
            const double u = step(a.r[q][i], a.u[q][i]);
            a.u[q][i] = u;
            if constexpr (DINV) if (q == J) a.gather[i] = a.dinv[i] * u;
        }
    };
    struct Pair { d2 r[J + 1], u[J + 1], d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {};
#pragma unroll
        for (int q = 0; q <= J; ++q) { e.r[q] = ldv<NTV>((const d2*)a.r[q] + i); e.u[q] = ldv<NTV>((const d2*)a.u[q] + i); }
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
#pragma unroll
        for (int q = 0; q <= J; ++q) {
            d2 o; o.x = step(e.r[q].x, e.u[q].x); o.y = step(e.r[q].y, e.u[q].y);
            stv<NTV>(o, (d2*)a.u[q] + i);
            if constexpr (DINV) if (q == J) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, (d2*)a.gather + i); }
        }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

template <bool V2, bool NTV, int HAT, int J>
__global__ __launch_bounds__(kBlock) void bicgstabl_r_kernel(BicgstablPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;
    __shared__ double s_red[4];
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if constexpr (J == 0) {                            // the first pass of a body
        const int done = a.f.sc->done;                 // nobody writes it while this pass runs
        if (publisher) { a.bs->fDone = done; for (int j = 0; j < kBicgstablMaxL; ++j) { a.bs->broke[j] = 0; a.bs->early[j] = 0; } }
        if (done != 0) return;
    } else {
        if (a.bs->fDone != 0 || bicgstabl_broke<J>(a.bs) || bicgstabl_early(a.bs)) return;
    }
    const double sigma = reduce_partials_block(a.in, a.nIn, s_red, 0);
    const double rho = a.bs->rho[a.k & 1][J];
    const double alpha = rho / sigma;
    if (sigma == 0.0 || !finite_value(sigma) || !finite_value(alpha)) {
        if (publisher) a.bs->broke[J] = 1;
        return;
    }
    if (publisher) { a.bs->alpha = alpha; a.f.sc->alpha = alpha; }
    __syncthreads();                                   // s_red is used again below
    double accR = 0.0;                                 // the new r_0.r_0, for the stop test in front of the next step
    auto step = [&](double r, double u) { double au = alpha * u; return r - au; };
    auto stepx = [&](double x, double u0, double d) { double h = u0; if constexpr (DINV) h = d * u0; double ah = alpha * h; return x + ah; };
    auto one = [&](long long i) {
        double d = 0.0;
        if constexpr (DINV) d = a.dinv[i];
        a.x[i] = stepx(a.x[i], a.u[0][i], d);
#pragma unroll
        for (int q = 0; q <= J; ++q) {
            const double r = step(a.r[q][i], a.u[q + 1][i]);
            a.r[q][i] = r;
            if (q == 0) { double sq = r * r; accR += sq; }
            if constexpr (DINV) if (q == J) a.gather[i] = d * r;
        }
    };
    struct Pair { d2 r[J + 1], u[J + 2], x, d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {};
        e.x = ldv<NTV>((const d2*)a.x + i);
#pragma unroll
        for (int q = 0; q <= J; ++q) e.r[q] = ldv<NTV>((const d2*)a.r[q] + i);
#pragma unroll
        for (int q = 0; q <= J + 1; ++q) e.u[q] = ldv<NTV>((const d2*)a.u[q] + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = stepx(e.x.x, e.u[0].x, e.d.x); o.y = stepx(e.x.y, e.u[0].y, e.d.y);
        stv<NTV>(o, (d2*)a.x + i);
#pragma unroll
        for (int q = 0; q <= J; ++q) {
            o.x = step(e.r[q].x, e.u[q + 1].x); o.y = step(e.r[q].y, e.u[q + 1].y);
            stv<NTV>(o, (d2*)a.r[q] + i);
            if (q == 0) { double s0 = o.x * o.x; double s1 = o.y * o.y; accR += s0; accR += s1; }
            if constexpr (DINV) if (q == J) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, (d2*)a.gather + i); }
        }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    const double sr = block_sum(accR, s_red);
    if (threadIdx.x == 0) a.outA[blockIdx.x] = sr;
}

// The partial sums of Z_ab = r_a.r_b, a = 1 .. L, b = 0 .. a: one read of r_0 .. r_L, region bicgstabl_entry(a, b) of `partials`.
template <bool V2, bool NTV, int L>
__global__ __launch_bounds__(kBlock) void bicgstabl_gram_kernel(BicgstablPass a, double* __restrict__ partials)
{
    constexpr int NE = L * (L + 3) / 2;
    __shared__ double s_red[NE][4];
    if (a.bs->fDone != 0 || bicgstabl_broke(a.bs) || bicgstabl_early(a.bs)) return;
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    auto add = [&](const double (&r)[L + 1]) {
#pragma unroll
        for (int p = 1; p <= L; ++p)
#pragma unroll
            for (int b = 0; b <= p; ++b) { double q = r[p] * r[b]; acc[bicgstabl_entry(p, b)] += q; }
    };
    grid_stride<V2>(a.n,
        [&](long long i) {
            double r0[L + 1], r1[L + 1];
#pragma unroll
            for (int q = 0; q <= L; ++q) { const d2 v = ldv<NTV>((const d2*)(a.r[q] + i)); r0[q] = v.x; r1[q] = v.y; }
            add(r0); add(r1);
        },
        [&](long long i) {
            double r0[L + 1];
#pragma unroll
            for (int q = 0; q <= L; ++q) r0[q] = a.r[q][i];
            add(r0);
        });
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const double sum = block_sum(acc[e], s_red[e]);
        if (threadIdx.x == 0) partials[(size_t)e * kMaxGrid + blockIdx.x] = sum;
    }
}

// gamma_1 .. gamma_L (g[0 .. L-1]) from Z, in the scalar order include/MgcgGpu.h fixes: the Cholesky factor C of G = Z[1..L, 1..L] row by row,
// m = the number of leading pivots that are > 0 and finite, C y = Z[1..m, 0] forwards, C^T gamma = y backwards, gamma_{m+1 .. L} = 0.  Every product
// goes into a double of its own.  Rows behind m are computed and never used: no branch leaves the unrolled loops.
template <int L>
__device__ __forceinline__ int bicgstabl_gamma(const double* Z, double* g)
{
    double C[L][L], y[L];
    int m = 0;
    bool live = true;
#pragma unroll
    for (int i = 0; i < L; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) {
            double s = Z[bicgstabl_entry(i + 1, j + 1)];
#pragma unroll
            for (int q = 0; q < j; ++q) { double t = C[i][q] * C[j][q]; s = s - t; }
            C[i][j] = s / C[j][j];
        }
        double s = Z[bicgstabl_entry(i + 1, i + 1)];
#pragma unroll
        for (int q = 0; q < i; ++q) { double t = C[i][q] * C[i][q]; s = s - t; }
        live = live && s > 0.0 && finite_value(s);
        if (live) m = i + 1;
        C[i][i] = sqrt(s);
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
        double s = Z[bicgstabl_entry(i + 1, 0)];
#pragma unroll
        for (int q = 0; q < i; ++q) { double t = C[i][q] * y[q]; s = s - t; }
        y[i] = s / C[i][i];
    }
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int q = i + 1; q < L; ++q) { double t = C[q][i] * g[q]; s = q < m ? s - t : s; }
        g[i] = i < m ? s / C[i][i] : 0.0;
    }
    return m;
}

template <bool V2, bool NTV, int HAT, int L>
__global__ __launch_bounds__(kBlock) void bicgstabl_combine_kernel(BicgstablPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;
    constexpr int NE = L * (L + 3) / 2;
    __shared__ double s_red[NE + 2][4];
    if (a.bs->fDone != 0 || bicgstabl_broke(a.bs) || bicgstabl_early(a.bs)) return;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    double Z[NE], g[L];
#pragma unroll
    for (int e = 0; e < NE; ++e) Z[e] = reduce_partials_block(a.in + (size_t)e * kMaxGrid, a.nIn, s_red[e], 0);
    const int m = bicgstabl_gamma<L>(Z, g);
    if (publisher) {
        a.bs->omega = g[L - 1]; a.bs->pivots = m;
#pragma unroll
        for (int j = 0; j < L; ++j) a.bs->gamma[j] = g[j];
    }
    double accR = 0.0, accH = 0.0;
    struct Elem { double u, x, r; };
    // one element: r[0 .. L], u[0 .. L], x, rt, d; the three sums term by term, j = 1 .. L, every product into a double of its own
    auto step = [&](const double (&r)[L + 1], const double (&u)[L + 1], double x, double rt, double d) {
        Elem o; o.u = u[0]; o.x = x; o.r = r[0];
#pragma unroll
        for (int j = 1; j <= L; ++j) { double t = g[j - 1] * u[j]; o.u = o.u - t; }
#pragma unroll
        for (int j = 1; j <= L; ++j) { double h = r[j - 1]; if constexpr (DINV) h = d * r[j - 1]; double t = g[j - 1] * h; o.x = o.x + t; }
#pragma unroll
        for (int j = 1; j <= L; ++j) { double t = g[j - 1] * r[j]; o.r = o.r - t; }
        double q = o.r * o.r; accR += q;
        double h = rt * o.r; accH += h;
        return o;
    };
    auto one = [&](long long i) {
        double r[L + 1], u[L + 1];
#pragma unroll
        for (int q = 0; q <= L; ++q) { r[q] = a.r[q][i]; u[q] = a.u[q][i]; }
        double d = 0.0;
        if constexpr (DINV) d = a.dinv[i];
        const Elem o = step(r, u, a.x[i], a.rt[i], d);
        a.u[0][i] = o.u; a.x[i] = o.x; a.r[0][i] = o.r;
    };
    struct Pair { d2 r[L + 1], u[L + 1], x, rt, d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {};
#pragma unroll
        for (int q = 0; q <= L; ++q) { e.r[q] = ldv<NTV>((const d2*)a.r[q] + i); e.u[q] = ldv<NTV>((const d2*)a.u[q] + i); }
        e.x = ldv<NTV>((const d2*)a.x + i); e.rt = ldv<NTV>((const d2*)a.rt + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        double r0[L + 1], r1[L + 1], u0[L + 1], u1[L + 1];
#pragma unroll
        for (int q = 0; q <= L; ++q) { r0[q] = e.r[q].x; r1[q] = e.r[q].y; u0[q] = e.u[q].x; u1[q] = e.u[q].y; }
        const Elem o0 = step(r0, u0, e.x.x, e.rt.x, e.d.x), o1 = step(r1, u1, e.x.y, e.rt.y, e.d.y);
        d2 o;
        o.x = o0.u; o.y = o1.u; stv<NTV>(o, (d2*)a.u[0] + i);
        o.x = o0.x; o.y = o1.x; stv<NTV>(o, (d2*)a.x + i);
        o.x = o0.r; o.y = o1.r; stv<NTV>(o, (d2*)a.r[0] + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    const double sr = block_sum(accR, s_red[NE]);
    const double sh = block_sum(accH, s_red[NE + 1]);
    if (threadIdx.x == 0) { a.outA[blockIdx.x] = sr; a.outB[blockIdx.x] = sh; }
}

template <bool V2, bool NTV, int HAT>
__global__ __launch_bounds__(kBlock) void bicgstabl_p_kernel(BicgstablPass a)
{
    constexpr bool DINV = HAT == HAT_DINV;
    __shared__ double s_red[4], s_red2[4];
    if (a.bs->fDone != 0) return;                      // the flag as pass R_0 found it: this pass raises the live one itself
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    if (bicgstabl_broke(a.bs)) {                       // sigma or alpha broke down in step j: x and r_0 are what steps 0 .. j-1 made them
        if (publisher) publish_breakdown(a.f, a.k + 1);
        return;
    }
    if (bicgstabl_early(a.bs)) {                       // r_0 met the stop test in front of a step: the body ended there
        if (publisher) {
            const double rrE = a.bs->rrEarly;
            const StopDecision d = decide_stop(a.f, rrE, 0.0, a.f.sc->rr0, a.k + 1);
            publish_iteration<0>(a.f, d, a.k + 1, rrE, 0.0, 0, [] {});
        }
        return;
    }
    const double rr = reduce_partials_block(a.in, a.nIn, s_red, 0);
    const double rhon = reduce_partials_block(a.inB, a.nIn, s_red2, 0);
    const int k = a.k;
    const double omega = a.bs->omega, alpha = a.bs->alpha, rho = a.bs->rho[k & 1][a.ell - 1];
    StopDecision d = decide_stop(a.f, rr, 0.0, a.f.sc->rr0, k + 1);
    if (!d.stop && (omega == 0.0 || rhon == 0.0 || !finite_value(rhon))) { d.stop = true; d.status = MGCG_NONFINITE; }   // x IS this body's iterate
    const double mo = -omega;
    const double den = mo * rho;
    const double q = rhon / den;
    const double beta = alpha * q;
    if (publisher) publish_iteration<0>(a.f, d, k + 1, rr, 0.0, 0, [&] { a.bs->rho[(k + 1) & 1][0] = rhon; a.f.sc->beta = beta; });
    if (d.stop) return;
    auto step = [&](double r, double u) { double bu = beta * u; return r - bu; };
    auto one = [&](long long i) {
        const double u = step(a.r[0][i], a.u[0][i]);
        a.u[0][i] = u;
        if constexpr (DINV) a.gather[i] = a.dinv[i] * u;
    };
    struct Pair { d2 r, u, d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {}; e.r = ldv<NTV>((const d2*)a.r[0] + i); e.u = ldv<NTV>((const d2*)a.u[0] + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = step(e.r.x, e.u.x); o.y = step(e.r.y, e.u.y);
        stv<NTV>(o, (d2*)a.u[0] + i);
        if constexpr (DINV) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, (d2*)a.gather + i); }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// The scalars in front of body 0 (one workgroup)
__global__ __launch_bounds__(kBlock) void bicgstabl_init_kernel(const double* __restrict__ partials, int n, FinalizeArgs f, BicgstablScalars* bs)
{
    __shared__ double s_red[4];
    const double rr0 = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    publish_start(f, rr0, sqrt(rr0));
    bs->red = 0.0; bs->alpha = 0.0; bs->omega = 0.0; bs->fDone = 0; bs->pivots = 0;
    for (int j = 0; j < kBicgstablMaxL; ++j) { bs->rho[0][j] = 0.0; bs->rho[1][j] = 0.0; bs->gamma[j] = 0.0; bs->broke[j] = 0; bs->early[j] = 0; }
    bs->rrEarly = 0.0;
    bs->rho[0][0] = rr0;
    if (!positive_finite(rr0)) refuse_start(f);        // b - A x is zero or not finite
}

void bicgstabl_enqueue_init(Workspace* ws, const FinalizeArgs& f, int nPartials)
{
    hipLaunchKernelGGL(bicgstabl_init_kernel, dim3(1), dim3(kBlock), 0, ws->stream, (const double*)bicgstab_rr_partials(ws), nPartials, f, ws->bicgstablScalars);
}

static BicgstablPass bicgstabl_pass_args(const BicgstablRun& R, const FinalizeArgs& f, int k)
{
    BicgstablPass a{};
    a.f = f; a.bs = R.ws->bicgstablScalars; a.k = k; a.ell = R.ell;
    a.x = R.x; a.rt = R.rt; a.dinv = R.dinv; a.gather = R.gather; a.n = R.n < 0 ? 0 : R.n;
    for (int j = 0; j <= kBicgstablMaxL; ++j) { a.r[j] = j <= R.ell ? R.r[j] : nullptr; a.u[j] = j <= R.ell ? R.u[j] : nullptr; }
    return a;
}

// every vector a pass may touch is 16-byte aligned
static bool bicgstabl_v2(const BicgstablRun& R)
{
    bool v2 = al16(R.x) && al16(R.rt) && al16(R.dinv) && al16(R.gather);
    for (int j = 0; j <= R.ell; ++j) v2 = v2 && al16(R.r[j]) && al16(R.u[j]);
    return v2;
}

// go(std::integral_constant<int, v>) for v = lo .. hi
template <int LO, int HI, typename Go> static void bicgstabl_with_int(int v, Go go)
{
    if constexpr (LO <= HI) {
        if (v == LO) go(std::integral_constant<int, LO>{});
        else bicgstabl_with_int<LO + 1, HI>(v, go);
    }
}

// go(V2, NTV, HAT) for the form this call takes
template <typename Go> static void bicgstabl_with_form(const BicgstablRun& R, bool v2, Go go)
{
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        with_hat(R.dinv, [&](auto HAT) { go(V2, NTV, HAT); });
    });
}

void bicgstabl_enqueue_u(const BicgstablRun& R, const FinalizeArgs& f, int k, int j, int nRho, int nRr)
{
    BicgstablPass a = bicgstabl_pass_args(R, f, k);
    a.in = R.ws->partials; a.nIn = nRho;
    a.inB = bicgstabl_partials(R.ws, kBicgstablGram); a.nInB = nRr;
    const bool v2 = bicgstabl_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstabl_with_form(R, v2, [&](auto V2, auto NTV, auto HAT) {
        bicgstabl_with_int<1, kBicgstablMaxL - 1>(j, [&](auto J) {
            hipLaunchKernelGGL((bicgstabl_u_kernel<V2.value, NTV.value, HAT.value, J.value>), dim3(grid), dim3(kBlock), 0, R.ws->stream, a);
        });
    });
}

int bicgstabl_enqueue_r(const BicgstablRun& R, const FinalizeArgs& f, int k, int j, int nSigma)
{
    BicgstablPass a = bicgstabl_pass_args(R, f, k);
    a.in = R.ws->partials; a.nIn = nSigma;
    a.outA = bicgstabl_partials(R.ws, kBicgstablGram);   // the combine pass's region: free while the steps run
    const bool v2 = bicgstabl_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstabl_with_form(R, v2, [&](auto V2, auto NTV, auto HAT) {
        bicgstabl_with_int<0, kBicgstablMaxL - 1>(j, [&](auto J) {
            hipLaunchKernelGGL((bicgstabl_r_kernel<V2.value, NTV.value, HAT.value, J.value>), dim3(grid), dim3(kBlock), 0, R.ws->stream, a);
        });
    });
    if (j + 1 >= R.ell) return grid;                   // the last step: the combine pass follows, nobody reads the sum
    if (dot_reference_order()) { launch_dot_serial(R.ws->stream, a.r[0], a.r[0], a.n, a.outA, &R.ws->scalars->done); return 1; }
    return grid;
}

int bicgstabl_enqueue_gram(const BicgstablRun& R)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.n < 0 ? 0 : R.n;
    if (dot_reference_order()) {                       // every entry in the reference's order
        const int* done = &ws->scalars->done;
        for (int p = 1; p <= R.ell; ++p)
            for (int b = 0; b <= p; ++b) launch_dot_serial(s, R.r[p], R.r[b], n, bicgstabl_partials(ws, bicgstabl_entry(p, b)), done);
        return 1;
    }
    FinalizeArgs none{};
    BicgstablPass a = bicgstabl_pass_args(R, none, 0);
    const bool v2 = bicgstabl_v2(R);
    const int grid = grid_for(n, v2 ? 4 : 2);
    with_v2_nt(v2, vec_nt(n), [&](auto V2, auto NTV) {
        bicgstabl_with_int<1, kBicgstablMaxL>(R.ell, [&](auto L) {
            hipLaunchKernelGGL((bicgstabl_gram_kernel<V2.value, NTV.value, L.value>), dim3(grid), dim3(kBlock), 0, s, a, bicgstabl_partials(ws, 0));
        });
    });
    return grid;
}

int bicgstabl_enqueue_combine(const BicgstablRun& R, const FinalizeArgs& f, int k, int nGram)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    BicgstablPass a = bicgstabl_pass_args(R, f, k);
    a.in = bicgstabl_partials(ws, 0); a.nIn = nGram;
    a.outA = bicgstabl_partials(ws, kBicgstablGram); a.outB = bicgstabl_partials(ws, kBicgstablGram + 1);
    const bool v2 = bicgstabl_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstabl_with_form(R, v2, [&](auto V2, auto NTV, auto HAT) {
        bicgstabl_with_int<1, kBicgstablMaxL>(R.ell, [&](auto L) {
            hipLaunchKernelGGL((bicgstabl_combine_kernel<V2.value, NTV.value, HAT.value, L.value>), dim3(grid), dim3(kBlock), 0, s, a);
        });
    });
    if (dot_reference_order()) {                       // r_0.r_0 and rt.r_0 in the reference's order
        const int* done = &ws->scalars->done;
        launch_dot_serial(s, a.r[0], a.r[0], a.n, a.outA, done);
        launch_dot_serial(s, a.rt, a.r[0], a.n, a.outB, done);
        return 1;
    }
    return grid;
}

void bicgstabl_enqueue_p(const BicgstablRun& R, const FinalizeArgs& f, int k, int nRr)
{
    Workspace* ws = R.ws;
    BicgstablPass a = bicgstabl_pass_args(R, f, k);
    a.in = bicgstabl_partials(ws, kBicgstablGram); a.inB = bicgstabl_partials(ws, kBicgstablGram + 1); a.nIn = nRr;
    const bool v2 = bicgstabl_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    bicgstabl_with_form(R, v2, [&](auto V2, auto NTV, auto HAT) {
        hipLaunchKernelGGL((bicgstabl_p_kernel<V2.value, NTV.value, HAT.value>), dim3(grid), dim3(kBlock), 0, ws->stream, a);
    });
}

void preload_kernels_bicgstabl() { preload_code_object(reinterpret_cast<const void*>(&bicgstabl_init_kernel)); }

} // namespace mgcg
