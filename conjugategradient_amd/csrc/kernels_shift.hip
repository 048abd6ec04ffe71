// Multi-shift CG for gfx950 (SolveShifted): (A + sigma_j I) x_j = b for k = 1..8 shifts sigma_j >= 0 from ONE CG recurrence on A.
//
// Krylov spaces are shift-invariant, so the residual of every shifted system is collinear with the base residual, r_j = zeta_j r, and an
// iteration needs the plain loop's product and r update (launch_spmv_auto, update_r_kernel: untouched) plus the one pass of this file.
// The base iterate is not stored; a caller who wants it lists the shift 0.
//
// Per base iteration k, behind update_r (alpha = alpha_k frozen, r = r_new, partial sums of r.r): beta = beta_k = r.r_new / r.r and, per
// live column j with zeta_{-1} = zeta_0 = 1, alpha_{-1} = 1, beta_{-1} = 0, p_j = b and x_j = 0 at the start,
//     zeta_new = zeta_k zeta_{k-1} alpha_{k-1} / ( alpha_{k-1} zeta_{k-1} (1 + sigma_j alpha_k) + alpha_k beta_{k-1} (zeta_{k-1} - zeta_k) )
//     alpha_j  = alpha_k (zeta_new / zeta_k)          beta_j = beta_k (zeta_new / zeta_k)^2
//     x_j = x_j + alpha_j p_j  (the old p_j)          p_j = zeta_new r_new + beta_j p_j          p = r_new + beta p
// Rounding contract (include/MgcgGpu.h): every product is rounded into a named double before the add that follows it, nothing is fused
// (-ffp-contract=off), and the scalar expressions are evaluated in exactly the order of shifted_scalars below.  For sigma = 0 that order
// gives zeta = 1.0, alpha_j = alpha and beta_j = beta exactly, so a shift-0 column is SolveEx's x bit for bit.
//
// The residual of column j is zeta_new^2 (r.r): decide_stop (common.hpp) sees rr_j = (zeta_new zeta_new) (r.r) and, for the max-norm
// rule, |zeta_new| max|r|, against the common r0.r0 = b.b.  No extra sums: under dot_order = 1 the loop's two dots are the serial ones.
//
// Scalar step: folded into the pass.  Every workgroup reduces update_r's partial sums in finalize_frozen's order and lanes 0..k-1 take
// one column each; the first workgroup alone publishes.  What the columns carry from one iteration to the next (zeta_k, zeta_{k-1},
// alpha_{k-1}, beta_{k-1}, live) is double-buffered by iteration parity (ShiftState, common.hpp), which is what update_r's frozen copies
// are to the plain loop: an iteration stays the product plus two launches.
//
// Column modes, as in block CG: 2 = x and p (the column goes on), 1 = x only (it stops in this iteration), 0 = frozen, none of its
// streams is touched.  A breakdown -- p.Ap <= 0 or not finite, a zeta_new, alpha_j or beta_j that is not finite -- ends the column with
// MGCG_NONFINITE and mode 0: its x keeps the last good iterate.  The device stop flag rises when no column is live.
#include "vec_passes.hpp"

namespace mgcg {

bool Workspace::ensure_shift()
{
    if (shiftScalars) return true;
    return MGCG_HIP(hipMalloc((void**)&shiftScalars, sizeof(ShiftScalars)));
}

// The scalars of one column for one iteration, in the contract's order: every product in a named double, then the add.
struct ShiftedColumn { double zeta, alpha, beta; };
__device__ __forceinline__ ShiftedColumn shifted_scalars(double sigma, double zetaK, double zetaPrev, double alphaPrev, double betaPrev, double alphaK, double betaK)
{
    const double t1 = zetaK * zetaPrev;
    const double num = t1 * alphaPrev;
    const double a1 = alphaPrev * zetaPrev;
    const double s1 = sigma * alphaK;
    const double s2 = 1.0 + s1;
    const double d1 = a1 * s2;
    const double b1 = alphaK * betaPrev;
    const double df = zetaPrev - zetaK;
    const double dd = b1 * df;
    const double den = d1 + dd;
    ShiftedColumn c;
    c.zeta = num / den;
    const double ratio = c.zeta / zetaK;
    c.alpha = alphaK * ratio;
    const double q = ratio * ratio;
    c.beta = betaK * q;
    return c;
}

// What the pass needs of the finalised iteration, the same in every lane of every workgroup.
template <int K>
struct ShiftedStep { double beta; double zeta[K], alpha[K], betaJ[K]; int mode[K]; bool anyLive; };

// The finalisation (see the head of the file).  Needs update_r launched with freeze = true.
template <int K>
__device__ __forceinline__ void shifted_finalize(const FinalizeArgs& f, ShiftScalars* sh, const double* partials, const double* partialsInf, int nPartials,
                                                 ShiftedStep<K>& out)
{
    __shared__ double s_red[4];
    __shared__ double s_red2[4];
    __shared__ double s_zeta[K], s_alpha[K], s_beta[K];
    __shared__ int s_mode[K], s_status[K];
    CgScalars* sc = f.sc;
    const double rrNew = reduce_partials_block(partials, nPartials, s_red, 0);
    const double inf = partialsInf != nullptr ? reduce_partials_block(partialsInf, nPartials, s_red2, 1) : 0.0;
    const int it = sc->fIteration;
    const double alpha = sc->fAlpha;
    const double beta = rrNew / sc->fRr;
    const double pAp = sc->pAp;                                        // (update_r's; nothing in this kernel writes it)
    const bool baseBroken = !(pAp > 0.0 && pAp <= 1.79e308);
    const ShiftState& cur = sh->st[it & 1];
    ShiftState& nxt = sh->st[(it + 1) & 1];
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        int mode = 0, status = MGCG_OK;
        ShiftedColumn c = { 0.0, 0.0, 0.0 };
        if (cur.live[j] != 0) {
            const double zetaK = cur.zeta[j];
            c = shifted_scalars(sh->sigma[j], zetaK, cur.zetaPrev[j], cur.alphaPrev, cur.betaPrev, alpha, beta);
            const double z2 = c.zeta * c.zeta;
            const double rrJ = z2 * rrNew;
            const double infJ = fabs(c.zeta) * inf;
            StopDecision d = decide_stop(f, rrJ, infJ, sc->fRr0, it);
            // (a zeta that underflowed to 0 is still finite; the iteration after it has ratio = 0 / 0, and is caught here by its alpha_j)
            const bool broken = baseBroken || !(fabs(c.zeta) <= 1.79e308) || !(fabs(c.alpha) <= 1.79e308) || !(fabs(c.beta) <= 1.79e308);
            if (broken) { d.stop = true; d.status = MGCG_NONFINITE; }
            mode = d.stop ? (broken ? 0 : 1) : 2;
            status = d.status;
            if (blockIdx.x == 0) {
                if (f.trace != nullptr && it < f.traceCap) f.trace[(long long)j * f.traceCap + it] = d.shown;
                nxt.zeta[j] = c.zeta; nxt.zetaPrev[j] = zetaK; nxt.live[j] = d.stop ? 0 : 1;
                if (d.stop) { sh->residual[j] = d.res; sh->iteration[j] = it; sh->status[j] = d.status; }
            }
        } else if (blockIdx.x == 0) {
            nxt.live[j] = 0;
        }
        s_zeta[j] = c.zeta; s_alpha[j] = c.alpha; s_beta[j] = c.beta; s_mode[j] = mode; s_status[j] = status;
    }
    __syncthreads();
    bool anyLive = false;
#pragma unroll
    for (int j = 0; j < K; ++j) { out.zeta[j] = s_zeta[j]; out.alpha[j] = s_alpha[j]; out.betaJ[j] = s_beta[j]; out.mode[j] = s_mode[j]; anyLive = anyLive || s_mode[j] == 2; }
    out.beta = beta; out.anyLive = anyLive;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the base recurrence goes on while a column is live; the call's status is the worst column's
        StopDecision d;
        d.res = f.rule == MGCG_RULE_HANDMADECL ? inf : sqrt(rrNew); d.shown = d.res; d.stop = !anyLive; d.status = MGCG_OK;
        for (int j = 0; j < K; ++j) {
            if (s_status[j] == MGCG_NONFINITE) d.status = MGCG_NONFINITE;
            else if (s_status[j] == MGCG_MAXIT_EXCEEDED && d.status == MGCG_OK) d.status = MGCG_MAXIT_EXCEEDED;
        }
        nxt.alphaPrev = alpha; nxt.betaPrev = beta;
        FinalizeArgs base = f;
        base.trace = nullptr;                                          // (the traces are per column, written above)
        publish_iteration<0>(base, d, it, rrNew, inf, 0, [&] { sc->beta = beta; sc->rr = rrNew; });
    }
}

// One base iteration's vector pass: r and p are read once; p = r + beta p; per column x_j = x_j + alpha_j p_j (mode >= 1) and
// p_j = zeta_j r + beta_j p_j (mode 2).  (3 + 4 k') 8 bytes per row with k' live columns.  V2: 16-byte accesses (every column of x and
// ps starts on a 16-byte boundary); NTV: the streaming hint of the loop's other passes, from the same size up (vec_nt).
template <int K, bool V2, bool NTV>
__global__ __launch_bounds__(kBlock) void update_shifted_kernel(FinalizeArgs f, ShiftScalars* sh, const double* __restrict__ partials, const double* __restrict__ partialsInf,
                                                                int nPartials, double* __restrict__ x, double* __restrict__ p, const double* __restrict__ r,
                                                                double* __restrict__ ps, long long n)
{
    if (f.sc->fDone != 0) return;                                      // the loop had stopped before this iteration: nothing ran, nothing is pending
    ShiftedStep<K> k;
    shifted_finalize<K>(f, sh, partials, partialsInf, nPartials, k);
    auto one = [&](long long i) {
        const double rv = r[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (k.mode[j] == 0) continue;
            double* xj = x + j * n; double* pj = ps + j * n;
            const double pv = pj[i]; double t = k.alpha[j] * pv; xj[i] = xj[i] + t;
            if (k.mode[j] == 2) { double u = k.zeta[j] * rv; double v = k.betaJ[j] * pv; pj[i] = u + v; }
        }
        if (k.anyLive) { double u = k.beta * p[i]; p[i] = rv + u; }
    };
    if constexpr (V2) {
        const d2* r2 = (const d2*)r; d2* p2 = (d2*)p;
        auto pair = [&](long long i) {
            d2 rv = ldv<NTV>(r2 + i), pv = {}, xv[K], qv[K];
            if (k.anyLive) pv = ldv<NTV>(p2 + i);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (k.mode[j] == 0) continue;
                xv[j] = ldv<NTV>((const d2*)(x + j * n) + i); qv[j] = ldv<NTV>((const d2*)(ps + j * n) + i);
            }
            if (k.anyLive) { double u0 = k.beta * pv.x; double u1 = k.beta * pv.y; pv.x = rv.x + u0; pv.y = rv.y + u1; stv<NTV>(pv, p2 + i); }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (k.mode[j] == 0) continue;
                double t0 = k.alpha[j] * qv[j].x; double t1 = k.alpha[j] * qv[j].y; xv[j].x = xv[j].x + t0; xv[j].y = xv[j].y + t1;
                stv<NTV>(xv[j], (d2*)(x + j * n) + i);
                if (k.mode[j] == 2) {
                    double u0 = k.zeta[j] * rv.x; double u1 = k.zeta[j] * rv.y; double v0 = k.betaJ[j] * qv[j].x; double v1 = k.betaJ[j] * qv[j].y;
                    qv[j].x = u0 + v0; qv[j].y = u1 + v1;
                    stv<NTV>(qv[j], (d2*)(ps + j * n) + i);
                }
            }
        };
        chunk_pairs(n >> 1, [&](long long i, bool two) { pair(i); if (two) pair(i + kBlock); });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
    } else {
        grid_stride<false>(n, [&](long long) {}, one);
    }
}

template <int K>
static void launch_update_shifted_k(hipStream_t s, const FinalizeArgs& f, ShiftScalars* sh, const double* partials, const double* partialsInf, int nPartials,
                                    double* x, double* p, const double* r, double* ps, long long n)
{
    // 16-byte accesses need every column to start on a 16-byte boundary: an even row count, or one column
    const bool v2 = al16(x) && al16(p) && al16(r) && al16(ps) && (K == 1 || (n & 1) == 0);
    with_v2_nt(v2, vec_nt(n), [&](auto V2, auto NTV) {
        hipLaunchKernelGGL((update_shifted_kernel<K, V2.value, NTV.value>), dim3(grid_for(n, V2.value ? 2 : 1)), dim3(kBlock), 0, s, f, sh, partials, partialsInf, nPartials,
                           x, p, r, ps, n);
    });
}

void launch_update_shifted(hipStream_t s, int k, const FinalizeArgs& f, ShiftScalars* sh, const double* partials, const double* partialsInf, int nPartials,
                           double* x, double* p, const double* r, double* ps, long long n)
{
    if (n <= 0) return;
    dispatch_k(k, [&](auto K) { launch_update_shifted_k<K.value>(s, f, sh, partials, partialsInf, nPartials, x, p, r, ps, n); });
}

void preload_kernels_shift() { preload_code_object(reinterpret_cast<const void*>(&update_shifted_kernel<1, false, false>)); }

} // namespace mgcg
