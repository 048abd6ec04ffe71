// Restarted GMRES(m) for gfx950 (SolveGmres / SolveGmresJacobi): Saad and Schultz's method for A x = b with A any CSR matrix, 1 <= m <= 32,
// right-preconditioned with M = I or M = diag(A), one rank.  An iteration is one Arnoldi step -- one product -- and a cycle is m of them; the
// residual never increases, the method cannot break down on a nonsingular matrix, and every restart recomputes r = b - A x by a product, so
// the judged figure cannot drift from the true one for longer than a cycle.  include/MgcgGpu.h has the method and its rounding contract;
// solver.hip's cg_solve_gmres the host's side.  Out of scope: several ranks, a non-flexible V-cycle form, m > 32, the C++ twin under host/.
//
// The V-cycle form (SolveGmresMg) is flexible GMRES on these kernels, none of them changed: the host enqueues a cycle z_j = M^-1 v_j in front
// of step j's product, straight into column j of a second block Z behind the basis (GmresRun::Z), the product gathers from that column, and
// the close hands Z to gmres_x_kernel as its column base: x += sum y_i z_i in the same groups, term order and rounding.  Everything between
// the product and the close works on V as before.  Its flag argument: the cycle and the product take the LIVE stop flag as their gate, which
// pass N alone raises and nobody writes while they run; a cycle enqueued behind a stop returns at the gate in every kernel and leaves z_{j+1}
// unwritten; the close reads columns below cols only, and column cols - 1 = j was written by the cycle in front of step j, with the flag
// down.  A cycle writes its column and the hierarchy's own iterates, never x, V, w or a scalar of the loop, so a work vector full of NaN on
// entry does not reach the result.  The close launches stay ungated and keyed on cols / yCount.
//
// The basis v_0 .. v_m lives in ONE work vector, column i at V + i * stride (and the gather buffer of the Jacobi form behind them); w is the
// caller's Ap vector.  The orthogonalisation is classical Gram-Schmidt applied `orth` times -- the j + 1 sums of a pass are independent, so
// they share launches and one reduction point, where modified Gram-Schmidt would need j + 1 dependent ones.  Step j of a cycle, c = j + 1
// columns in q = ceil(c / 8) launches; vectors read + written:
//     product   launch_spmv_auto          w = A hat(v_j)                                                  (the plain loop's)
//     dots      gmres_dots_kernel         the partial sums of v_i.w, at most 8 columns per launch, region i of kMaxGrid doubles: w is read
//                                         once per launch                                                                      c + q
//     fold      gmres_fold_kernel         one workgroup per entry: h'_i = the sum of region i; the second pass also h_i += h'_i    -
//     update    gmres_update_kernel       w -= sum h'_i v_i, at most 8 columns per launch; the last launch of the last pass also leaves
//                                         the partial sums of w.w                                                              c + 2 q
//     pass N    gmres_n_kernel            hn^2 = w.w ; the stored rotations on h ; the new rotation ; the stop decision ; v_{j+1} = w / hn
//                                         (and gather = dinv v_{j+1})                                                          2 / 4
// and per cycle
//     close     gmres_solve_kernel        one workgroup: y = R^-1 g over the `cols` completed columns ; yCount = cols ; cols = 0     -
//               gmres_x_kernel            x += hat(sum y_i v_i), at most 8 columns per launch; ceil(m / 8) launches are always enqueued and
//                                         those at or beyond yCount return                                      cols + 2 ceil(cols / 8)
//     restart   launch_spmv_auto, the r.r sums, gmres_restart_kernel: r = b - A x ; beta ; v_0 = r / beta ; g_0 = beta     a product + 2 / 4
// Averaged over a cycle of m = 20 that is 8 x (orth x 26.4 + 2 + 1.3 + 0.15) = about 240 bytes per row per step with orth = 1 and about 450
// with orth = 2; a 7-point product adds about 104 (and the restart's a twentieth of that).  BiCGStab moves about 164 per product and BiCGStab(2) about 180: this loop is slower per
// product than both.  It buys robustness, not bytes.
// The fold launch is there because 33 regions of up to 2048 partial sums, added redundantly by each of 2048 workgroups of a pass, would be about
// 1 GiB of L2 traffic per step; one workgroup per entry reads each region once.  Pass N, in contrast, is redundant: every workgroup adds the one
// region of w.w, rotates the at most 33 entries of h in LDS (a few hundred scalar operations on one lane) and takes the same stop decision from
// the same numbers in the same order; the first workgroup alone persists the column of R, c, s, g, cols = j + 1, the trace entry and the host
// mirror.  All scalars stay on the device (GmresScalars).
//
// The stop flag is CgScalars::done, and pass N alone raises it.  The first launch of a step -- the first dots launch, under dot_order = 1
// gmres_freeze_kernel -- copies the flag as it found it into GmresScalars::fDone; every later launch of the step looks at the copy, never at
// the live flag, which pass N raises while its other workgroups may still start.  The products and the restart launches are gated on the live
// flag: nobody writes it while they run.  A restart whose r.r is zero or not finite writes no vector in any workgroup -- all of them take the
// same decision from the same sum -- and its first workgroup leaves GmresScalars::note, which only LATER launches read: the passes of the next
// step return at it and its pass N publishes the end.  Pass N reads g_j from gLast[k & 1] and its first workgroup writes g_{j+1} to
// gLast[(k + 1) & 1], c_j, s_j and column j of R, which no workgroup of the same launch reads.  So no workgroup ever reads a scalar that a
// workgroup of the same launch writes.
// The close launches are NOT gated on the stop flag: they are keyed on cols and yCount.  The host enqueues them in front of every restart and
// once more behind the loop; the first of them that finds cols > 0 applies the cycle's columns and sets cols = 0, every other one does nothing.
// Whatever was enqueued behind the stop, x is therefore updated exactly once per cycle -- the cycle cut short by a stop, the cap or a breakdown
// included.  No launch reads a column, an entry of h or an entry of y at or beyond its live count: the counts are uniform, the predicates skip
// the load itself, and a work vector full of NaN on entry never meets a multiplication by 0.
//
// Same grid, chunked 16-byte accesses and streaming hints as kernels_bicgstabl.hip (vec_passes.hpp); every product goes into a named double
// before the add or subtraction that follows it (-ffp-contract=off).  Under dot_order = 1 every sum is launch_dot_serial's, and the loop is a
// fixed sequence of IEEE operations (tests/test_gmres_host.py restates it in numpy).
#include "vec_passes.hpp"

namespace mgcg {

constexpr int kGmresGroup = 8;                         // columns per dots / update / x launch
constexpr int kGmresWw = kGmresMaxM;                   // the region of w.w, of the start's and every restart's r.r and of the closing r.r

bool Workspace::ensure_gmres()
{
    if (!gmresScalars && !MGCG_HIP(hipMalloc((void**)&gmresScalars, sizeof(GmresScalars)))) return false;
    if (!gmresPartials && !MGCG_HIP(hipMalloc((void**)&gmresPartials, sizeof(double) * (size_t)(kGmresMaxM + 1) * kMaxGrid))) return false;
    return true;
}

// Region e of the loop's own partial sums: e < kGmresMaxM the sums of v_e.w, then kGmresWw.
static double* gmres_partials(Workspace* ws, int e) { return ws->gmresPartials + (size_t)e * kMaxGrid; }
double* gmres_rr_partials(Workspace* ws) { return gmres_partials(ws, kGmresWw); }

struct GmresPass {
    FinalizeArgs f;
    GmresScalars* gs;
    const double* in; int nIn;                         // the partial sums in front of the launch: fold the regions of v_i.w; pass N w.w; restart r.r
    double* out;                                       // dots: region c0; the last update launch: w.w
    int k, j;                                          // the step's index -- the host's count, which is the device's while the loop is live -- and k mod m
    int c0, cnt;                                       // this launch's columns c0 .. c0 + cnt - 1 (cnt <= kGmresGroup)
    int first;                                         // dots: the first launch of the step; fold: the first pass; restart: the start
    double *x, *w, *V, *gather;
    const double *r, *dinv;
    long long stride, n;
};

// dot_order = 1: the first launch of a step, in place of the first dots launch
__global__ void gmres_freeze_kernel(const CgScalars* sc, GmresScalars* gs) { gs->fDone = sc->done; }

// The partial sums of v_i.w, i = c0 .. c0 + cnt - 1, into regions 0 .. cnt - 1 of `out`; cnt is uniform, columns at or beyond it are not read.
template <bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void gmres_dots_kernel(GmresPass a)
{
    __shared__ double s_red[kGmresGroup][4];
    if (a.first) {
        const int done = a.f.sc->done;                 // nobody writes it while this launch runs
        if (blockIdx.x == 0 && threadIdx.x == 0) a.gs->fDone = done;
        if (done != 0) return;
    } else if (a.gs->fDone != 0) return;
    if (a.gs->note != 0) return;
    const double* v0 = a.V + (long long)a.c0 * a.stride;
    const int cnt = a.cnt;
    double acc[kGmresGroup];
#pragma unroll
    for (int q = 0; q < kGmresGroup; ++q) acc[q] = 0.0;
    grid_stride<V2>(a.n,
        [&](long long i) {
            const d2 w = ldv<NTV>((const d2*)(a.w + i));
#pragma unroll
            for (int q = 0; q < kGmresGroup; ++q)
                if (q < cnt) {
                    const d2 v = ldv<NTV>((const d2*)(v0 + q * a.stride + i));
                    double p0 = v.x * w.x; acc[q] += p0;
                    double p1 = v.y * w.y; acc[q] += p1;
                }
        },
        [&](long long i) {
            const double w = a.w[i];
#pragma unroll
            for (int q = 0; q < kGmresGroup; ++q)
                if (q < cnt) { double p = v0[q * a.stride + i] * w; acc[q] += p; }
        });
#pragma unroll
    for (int q = 0; q < kGmresGroup; ++q)
        if (q < cnt) {
            const double sum = block_sum(acc[q], s_red[q]);
            if (threadIdx.x == 0) a.out[(size_t)q * kMaxGrid + blockIdx.x] = sum;
        }
}

// Workgroup i: h'_i = the sum of region i; the first pass h_i = h'_i, the second h_i = h_i + h'_i
__global__ __launch_bounds__(kBlock) void gmres_fold_kernel(GmresPass a)
{
    __shared__ double s_red[4];
    if (a.gs->fDone != 0 || a.gs->note != 0) return;
    const int i = blockIdx.x;
    const double sum = reduce_partials_block(a.in + (size_t)i * kMaxGrid, a.nIn, s_red, 0);
    if (threadIdx.x == 0) {
        a.gs->hp[i] = sum;
        a.gs->h[i] = a.first ? sum : a.gs->h[i] + sum;
    }
}

// w = ((w - h'_c0 v_c0) - h'_{c0+1} v_{c0+1}) - ... over this launch's columns; SUMS: the partial sums of the new w.w
template <bool V2, bool NTV, bool SUMS>
__global__ __launch_bounds__(kBlock) void gmres_update_kernel(GmresPass a)
{
    __shared__ double s_red[4];
    if (a.gs->fDone != 0 || a.gs->note != 0) return;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const double* v0 = a.V + (long long)a.c0 * a.stride;
    const int cnt = a.cnt;
    double hp[kGmresGroup];
#pragma unroll
    for (int q = 0; q < kGmresGroup; ++q) hp[q] = q < cnt ? a.gs->hp[a.c0 + q] : 0.0;
    double accW = 0.0;
    auto one = [&](long long i) {
        double w = a.w[i];
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) { double t = hp[q] * v0[q * a.stride + i]; w = w - t; }
        a.w[i] = w;
        if constexpr (SUMS) { double sq = w * w; accW += sq; }
    };
    struct Pair { d2 w, v[kGmresGroup]; };
    auto load = [&](Pair& e, long long i) {
        e.w = ldv<NTV>((const d2*)a.w + i);
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) e.v[q] = ldv<NTV>((const d2*)(v0 + q * a.stride) + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o = e.w;
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) {
                double t0 = hp[q] * e.v[q].x; o.x = o.x - t0;
                double t1 = hp[q] * e.v[q].y; o.y = o.y - t1;
            }
        stv<NTV>(o, (d2*)a.w + i);
        if constexpr (SUMS) { double s0 = o.x * o.x; double s1 = o.y * o.y; accW += s0; accW += s1; }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
    if constexpr (SUMS) {
        const double sw = block_sum(accW, s_red);
        if (threadIdx.x == 0) a.out[blockIdx.x] = sw;
    }
}

// What ends the loop without a judged figure of its own (one thread): status, the residual to report, for iteration `it`
__device__ __forceinline__ void gmres_publish_end(const FinalizeArgs& f, int status, double res, int it)
{
    CgScalars* sc = f.sc;
    sc->residual = res; sc->done = 1; sc->status = status;
    f.mirror->residual = res; f.mirror->iteration = it; f.mirror->status = status;
    __threadfence_system();
    f.mirror->done = 1;
}

template <bool V2, bool NTV, bool DINV>
__global__ __launch_bounds__(kBlock) void gmres_n_kernel(GmresPass a)
{
    __shared__ double s_red[4];
    __shared__ double s_h[kGmresMaxM], s_c[kGmresMaxM], s_s[kGmresMaxM];
    __shared__ double s_hn;
    __shared__ int s_end;
    GmresScalars* gs = a.gs;
    if (gs->fDone != 0) return;                        // the flag as the first launch of the step found it: this pass raises the live one itself
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const int j = a.j, k = a.k;
    if (gs->note != 0) {                               // the restart in front of this step found r.r zero (1) or not finite (2): k steps were made
        if (publisher) {
            if (gs->note == 1) gmres_publish_end(a.f, MGCG_OK, 0.0, k);
            else gmres_publish_end(a.f, MGCG_NONFINITE, a.f.sc->residual, k);
        }
        return;
    }
    const double hn2 = reduce_partials_block(a.in, a.nIn, s_red, 0);
    if ((int)threadIdx.x <= j) s_h[threadIdx.x] = gs->h[threadIdx.x];
    if ((int)threadIdx.x < j) { s_c[threadIdx.x] = gs->cs[threadIdx.x]; s_s[threadIdx.x] = gs->sn[threadIdx.x]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < j; ++i) {                  // the stored rotations
            const double c = s_c[i], s = s_s[i], hi = s_h[i], hi1 = s_h[i + 1];
            double t1 = c * hi, t2 = s * hi1, t3 = s * hi, t4 = c * hi1;
            s_h[i] = t1 + t2;
            s_h[i + 1] = t4 - t3;
        }
        const double hn = sqrt(hn2);
        const double hjj = s_h[j];
        double p1 = hjj * hjj, p2 = hn * hn;
        const double dd = p1 + p2;
        const double d = sqrt(dd);
        if (!finite_value(hn2) || d == 0.0 || !finite_value(d)) {   // no next direction and no column: the last judged figure once more, for iteration k + 1
            if (publisher) publish_breakdown(a.f, k + 1);
            s_end = 1;
        } else {
            const double c = hjj / d, s = hn / d;
            const double gj = gs->gLast[k & 1];
            const double ms = -s;
            const double gn = ms * gj;
            const double gjn = c * gj;
            const double gg = gn * gn;
            StopDecision e = decide_stop(a.f, gg, 0.0, a.f.sc->rr0, k + 1);
            if (hn2 == 0.0) { e.stop = true; e.status = MGCG_OK; }   // the Krylov space is exhausted: x will be exact, whatever minIteration says
            if (publisher) {
                for (int i = 0; i < j; ++i) gs->R[i][j] = s_h[i];
                gs->R[j][j] = d; gs->cs[j] = c; gs->sn[j] = s; gs->g[j] = gjn; gs->gLast[(k + 1) & 1] = gn; gs->cols = j + 1;
                publish_iteration<0>(a.f, e, k + 1, gg, 0.0, 0, [] {});
            }
            s_end = e.stop ? 1 : 0;
            s_hn = hn;
        }
    }
    __syncthreads();
    if (s_end != 0) return;
    const double hn = s_hn;
    double* vn = a.V + (long long)(j + 1) * a.stride;
    auto one = [&](long long i) {
        const double v = a.w[i] / hn;
        vn[i] = v;
        if constexpr (DINV) a.gather[i] = a.dinv[i] * v;
    };
    struct Pair { d2 w, d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {}; e.w = ldv<NTV>((const d2*)a.w + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = e.w.x / hn; o.y = e.w.y / hn;
        stv<NTV>(o, (d2*)vn + i);
        if constexpr (DINV) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, (d2*)a.gather + i); }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// The scalars in front of step 0 (one workgroup), from the partial sums of the first r.r
__global__ __launch_bounds__(kBlock) void gmres_init_kernel(const double* __restrict__ partials, int n, FinalizeArgs f, GmresScalars* gs)
{
    __shared__ double s_red[4];
    const double rr0 = reduce_partials_block(partials, n, s_red, 0);
    if (threadIdx.x != 0) return;
    publish_start(f, rr0, sqrt(rr0));
    gs->red = 0.0; gs->gLast[0] = 0.0; gs->gLast[1] = 0.0; gs->fDone = 0; gs->note = 0; gs->cols = 0; gs->yCount = 0;
    if (!positive_finite(rr0)) refuse_start(f);        // b - A x is zero or not finite
}

// beta = sqrt(r.r) ; v_0 = r / beta ; gather = dinv v_0 ; g_0 = beta, where step k will look for it.  Gated on the live flag.
template <bool V2, bool NTV, bool DINV>
__global__ __launch_bounds__(kBlock) void gmres_restart_kernel(GmresPass a)
{
    __shared__ double s_red[4];
    if (a.f.sc->done != 0) return;                     // nobody writes it while this launch runs
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const double beta2 = reduce_partials_block(a.in, a.nIn, s_red, 0);
    if (!a.first && (beta2 == 0.0 || !finite_value(beta2))) {   // (the start's own r.r was judged by gmres_init_kernel)
        if (publisher) a.gs->note = beta2 == 0.0 ? 1 : 2;
        return;
    }
    const double beta = sqrt(beta2);
    if (publisher) a.gs->gLast[a.k & 1] = beta;
    auto one = [&](long long i) {
        const double v = a.r[i] / beta;
        a.V[i] = v;
        if constexpr (DINV) a.gather[i] = a.dinv[i] * v;
    };
    struct Pair { d2 r, d; };
    auto load = [&](Pair& e, long long i) {
        e.d = {}; e.r = ldv<NTV>((const d2*)a.r + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 o; o.x = e.r.x / beta; o.y = e.r.y / beta;
        stv<NTV>(o, (d2*)a.V + i);
        if constexpr (DINV) { d2 h; h.x = e.d.x * o.x; h.y = e.d.y * o.y; stv<NTV>(h, (d2*)a.gather + i); }
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

// The close's first launch (one workgroup, not gated): y = R^-1 g over the completed columns, backwards; yCount = cols ; cols = 0
__global__ __launch_bounds__(kBlock) void gmres_solve_kernel(GmresScalars* gs)
{
    __shared__ double s_R[kGmresMaxM][kGmresMaxM + 1], s_g[kGmresMaxM], s_y[kGmresMaxM];
    const int cols = gs->cols;                         // uniform: this launch's one workgroup writes it behind the last read
    if (cols > 0) {
        for (int e = threadIdx.x; e < cols * cols; e += kBlock) {
            const int i = e / cols, q = e % cols;
            if (q >= i) s_R[i][q] = gs->R[i][q];
        }
        if ((int)threadIdx.x < cols) s_g[threadIdx.x] = gs->g[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = cols - 1; i >= 0; --i) {
                double acc = s_g[i];
                for (int q = i + 1; q < cols; ++q) { double t = s_R[i][q] * s_y[q]; acc = acc - t; }
                s_y[i] = acc / s_R[i][i];
            }
        __syncthreads();
        if ((int)threadIdx.x < cols) gs->y[threadIdx.x] = s_y[threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) { gs->yCount = cols; gs->cols = 0; }
}

// x += hat(((0 + y_c0 v_c0) + y_{c0+1} v_{c0+1}) + ...) over the columns of this launch that lie below yCount (not gated)
template <bool V2, bool NTV, bool DINV>
__global__ __launch_bounds__(kBlock) void gmres_x_kernel(GmresPass a)
{
    const int left = a.gs->yCount - a.c0;
    if (left <= 0) return;
    const int cnt = left < kGmresGroup ? left : kGmresGroup;
    const bool publisher = blockIdx.x == 0 && threadIdx.x == 0;
    const double* v0 = a.V + (long long)a.c0 * a.stride;
    double y[kGmresGroup];
#pragma unroll
    for (int q = 0; q < kGmresGroup; ++q) y[q] = q < cnt ? a.gs->y[a.c0 + q] : 0.0;
    auto one = [&](long long i) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) { double p = y[q] * v0[q * a.stride + i]; acc = acc + p; }
        double h = acc;
        if constexpr (DINV) h = a.dinv[i] * acc;
        a.x[i] = a.x[i] + h;
    };
    struct Pair { d2 x, d, v[kGmresGroup]; };
    auto load = [&](Pair& e, long long i) {
        e.d = {}; e.x = ldv<NTV>((const d2*)a.x + i);
        if constexpr (DINV) e.d = ldv<NTV>((const d2*)a.dinv + i);
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) e.v[q] = ldv<NTV>((const d2*)(v0 + q * a.stride) + i);
    };
    auto finish = [&](const Pair& e, long long i) {
        d2 acc; acc.x = 0.0; acc.y = 0.0;
#pragma unroll
        for (int q = 0; q < kGmresGroup; ++q)
            if (q < cnt) {
                double p0 = y[q] * e.v[q].x; acc.x = acc.x + p0;
                double p1 = y[q] * e.v[q].y; acc.y = acc.y + p1;
            }
        d2 h = acc;
        if constexpr (DINV) { h.x = e.d.x * acc.x; h.y = e.d.y * acc.y; }
        d2 o; o.x = e.x.x + h.x; o.y = e.x.y + h.y;
        stv<NTV>(o, (d2*)a.x + i);
    };
    stream_pairs<V2, Pair>(a.n, publisher, load, finish, one);
}

static GmresPass gmres_pass_args(const GmresRun& R, const FinalizeArgs& f, int k, int j)
{
    GmresPass a{};
    a.f = f; a.gs = R.ws->gmresScalars; a.k = k; a.j = j;
    a.x = R.x; a.w = R.w; a.V = R.V; a.gather = R.gather; a.r = R.r; a.dinv = R.dinv; a.stride = R.stride; a.n = R.n < 0 ? 0 : R.n;
    return a;
}

// every vector a pass may touch is 16-byte aligned (the columns lie an even number of entries apart)
static bool gmres_v2(const GmresRun& R) { return al16(R.x) && al16(R.w) && al16(R.V) && al16(R.Z) && al16(R.gather) && al16(R.r) && al16(R.dinv) && (R.stride & 1) == 0; }

// go(V2, NTV, DINV) for the form this call takes
template <typename Go> static void gmres_with_form(const GmresRun& R, bool v2, Go go)
{
    with_v2_nt(v2, vec_nt(R.n), [&](auto V2, auto NTV) {
        if (R.dinv) go(V2, NTV, std::true_type{});
        else go(V2, NTV, std::false_type{});
    });
}

void gmres_enqueue_init(const GmresRun& R, const FinalizeArgs& f, int nPartials)
{
    hipLaunchKernelGGL(gmres_init_kernel, dim3(1), dim3(kBlock), 0, R.ws->stream, (const double*)gmres_rr_partials(R.ws), nPartials, f, R.ws->gmresScalars);
}

void gmres_enqueue_restart(const GmresRun& R, const FinalizeArgs& f, int k, int nRr, bool first)
{
    GmresPass a = gmres_pass_args(R, f, k, 0);
    a.in = gmres_rr_partials(R.ws); a.nIn = nRr; a.first = first ? 1 : 0;
    const bool v2 = gmres_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    gmres_with_form(R, v2, [&](auto V2, auto NTV, auto DINV) {
        hipLaunchKernelGGL((gmres_restart_kernel<V2.value, NTV.value, DINV.value>), dim3(grid), dim3(kBlock), 0, R.ws->stream, a);
    });
}

void gmres_enqueue_step(const GmresRun& R, const FinalizeArgs& f, int k, int j)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    GmresScalars* gs = ws->gmresScalars;
    const bool ref = dot_reference_order();
    const bool v2 = gmres_v2(R);
    const bool nt = vec_nt(R.n);
    const int cols = j + 1, groups = (cols + kGmresGroup - 1) / kGmresGroup;
    const int gridDots = grid_for(R.n, v2 ? 4 : 2), grid = grid_for(R.n, v2 ? 2 : 1);
    GmresPass a = gmres_pass_args(R, f, k, j);
    int nWw = grid;
    for (int pass = 0; pass < R.orth; ++pass) {
        int nDots = gridDots;
        if (ref) {                                     // every sum in the reference's order
            if (pass == 0) hipLaunchKernelGGL(gmres_freeze_kernel, dim3(1), dim3(1), 0, s, (const CgScalars*)ws->scalars, gs);
            for (int i = 0; i < cols; ++i) launch_dot_serial(s, R.V + i * R.stride, R.w, a.n, gmres_partials(ws, i), &gs->fDone);
            nDots = 1;
        } else {
            for (int g = 0; g < groups; ++g) {
                GmresPass d = a;
                d.c0 = g * kGmresGroup; d.cnt = cols - d.c0 < kGmresGroup ? cols - d.c0 : kGmresGroup;
                d.first = (pass == 0 && g == 0) ? 1 : 0; d.out = gmres_partials(ws, d.c0);
                with_v2_nt(v2, nt, [&](auto V2, auto NTV) {
                    hipLaunchKernelGGL((gmres_dots_kernel<V2.value, NTV.value>), dim3(gridDots), dim3(kBlock), 0, s, d);
                });
            }
        }
        GmresPass fo = a;
        fo.in = gmres_partials(ws, 0); fo.nIn = nDots; fo.first = pass == 0 ? 1 : 0;
        hipLaunchKernelGGL(gmres_fold_kernel, dim3(cols), dim3(kBlock), 0, s, fo);
        for (int g = 0; g < groups; ++g) {
            GmresPass u = a;
            u.c0 = g * kGmresGroup; u.cnt = cols - u.c0 < kGmresGroup ? cols - u.c0 : kGmresGroup; u.out = gmres_partials(ws, kGmresWw);
            const bool sums = !ref && pass == R.orth - 1 && g == groups - 1;
            with_v2_nt(v2, nt, [&](auto V2, auto NTV) {
                if (sums) hipLaunchKernelGGL((gmres_update_kernel<V2.value, NTV.value, true>), dim3(grid), dim3(kBlock), 0, s, u);
                else hipLaunchKernelGGL((gmres_update_kernel<V2.value, NTV.value, false>), dim3(grid), dim3(kBlock), 0, s, u);
            });
        }
    }
    if (ref) { launch_dot_serial(s, R.w, R.w, a.n, gmres_partials(ws, kGmresWw), &gs->fDone); nWw = 1; }
    a.in = gmres_partials(ws, kGmresWw); a.nIn = nWw;
    gmres_with_form(R, v2, [&](auto V2, auto NTV, auto DINV) {
        hipLaunchKernelGGL((gmres_n_kernel<V2.value, NTV.value, DINV.value>), dim3(grid), dim3(kBlock), 0, s, a);
    });
}

void gmres_enqueue_close(const GmresRun& R)
{
    hipStream_t s = R.ws->stream;
    hipLaunchKernelGGL(gmres_solve_kernel, dim3(1), dim3(kBlock), 0, s, R.ws->gmresScalars);
    FinalizeArgs none{};
    GmresPass a = gmres_pass_args(R, none, 0, 0);
    if (R.Z) a.V = R.Z;                                // the flexible form: the same pass over the stored z_i, x += sum y_i z_i
    const bool v2 = gmres_v2(R);
    const int grid = grid_for(R.n, v2 ? 2 : 1);
    for (int c0 = 0; c0 < R.m; c0 += kGmresGroup) {
        a.c0 = c0;
        gmres_with_form(R, v2, [&](auto V2, auto NTV, auto DINV) {
            hipLaunchKernelGGL((gmres_x_kernel<V2.value, NTV.value, DINV.value>), dim3(grid), dim3(kBlock), 0, s, a);
        });
    }
}

void preload_kernels_gmres() { preload_code_object(reinterpret_cast<const void*>(&gmres_init_kernel)); }

} // namespace mgcg
