// Solver half of the C ABI: the whole CG / preconditioned-CG loop, resident on the device.
// Replaces Mgcg/cuBlas/MgcgGpu/Mgcg.cu:201-270 (Solve) and the host-driven multi-device loop of
// Mgcg/cuBlas/Mgcg/ConjugateGradientParallelGpu.cs:424-565.
//
// Per iteration the reference issues 7 library calls and 2 blocking 8-byte device->host reads.
// Here an iteration is 3 streaming kernels + 2 single-workgroup scalar kernels, alpha / beta /
// the stop test live in device memory, and the host only enqueues: it runs `checkEvery` iterations
// ahead and looks at a pinned flag the device wrote.  Once the stop test fires on the device every
// later kernel exits at its first instruction, so x, r, p, Iteration and Residual are exactly those
// of the iteration the reference would have stopped at.
#include "common.hpp"
#include <algorithm>
#include <chrono>
#include <functional>

namespace mgcg {

// ---------------------------------------------------------------- multigrid hierarchy
// Every level lives on the rank's z-slab [z0, z1) of that level's grid: local CSR rows with GLOBAL column ids,
// local rhs / residual / D^-1, and two FULL-length iterate buffers (like p in the CG loop) whose halo planes are
// exchanged before every SpMV-shaped pass.  A single rank is the special case z0 = 0, z1 = nz.
struct MgLevel {
    int nx = 0, ny = 0, nz = 0;            // global grid of the level
    int z0 = 0, z1 = 0;                    // this rank's planes
    long long n = 0, nnz = 0;              // local rows / nonzeros
    long long nGlobal = 0, offset = 0;     // global rows, first local row
    double* elements = nullptr; int* rowOffsets = nullptr; int* columnIndeces = nullptr;
    bool ownsMatrix = false;
    double* dinv = nullptr;
    bool dinvUniform = false; double dinvScalar = 0.0;   // every diagonal equal: the kernels use the scalar and skip the array
    double *xa = nullptr, *xb = nullptr;   // iterate ping-pong, full length (Jacobi is not in place)
    double *b = nullptr, *r = nullptr;     // right-hand side (restricted residual), residual; local
    SpmvConfig cfg;                        // per level: kernel picked from its nnz/row, banded period = nx*ny
    const DcsrMatrix* dcsr = nullptr;      // compressed form (owned by the MgcgSparse handle's cache)
    HaloPlan* halo = nullptr;              // multi-rank: planes of the iterate owned by the neighbours
    HaloPlan* transferHalo = nullptr;      // multi-rank, linear transfer: exactly one grid plane from each z-neighbour
    int minJ = 0, maxJ = -1;
    bool overlap = false;                  // interior rows [interior0, interior1) are multiplied while the halo travels
    long long interior0 = 0, interior1 = 0;
    // Deep-halo cycle (several ranks, levels >= 1; mg_deep_level below): the right-hand side lives in a FULL-length buffer whose `deep`
    // planes either side of the slab arrive in ONE exchange per cycle (bHalo), and the level's matrix rows, right-hand side and D^-1 for
    // those planes are here too (copied from the neighbours at set-up), so that the sweeps can be recomputed on them instead of exchanged.
    int deep = 0;                          // planes either side (0: the level takes one exchange per sweep)
    int extZ0 = 0, extZ1 = 0;              // planes [extZ0, extZ1) of the extended slab (clipped to the grid)
    double* bFull = nullptr;               // b = bFull + offset
    HaloPlan* bHalo = nullptr;
    double* extElements = nullptr; int* extRowOffsets = nullptr; int* extColumnIndeces = nullptr; double* extDinv = nullptr;
    long long extRows = 0, extNnz = 0, extBase = 0;   // rows of the extended slab, its nonzeros, global index of its first row
    // Aggregation hierarchy (MgSetupAggregation / MgSetupAggregates; one rank), every level but the last: the map to the next level and its
    // inverted index.  Such a level is a "grid" of n x 1 x 1 cells, and a level that has a map never reaches the grid-addressed kernels.
    int* agg = nullptr;                    // n: row -> aggregate
    int* aggOffsets = nullptr;             // rows of the next level + 1
    int* aggMembers = nullptr;             // n: the members of aggregate I, ascending, at [aggOffsets[I], aggOffsets[I + 1])
    // Multicolour Gauss-Seidel smoother (MgSetSmoother(mg, 1); every level of an aggregation hierarchy): the rows of colour c, ascending,
    // are gsRows[gsOffsets[c] .. gsOffsets[c + 1])
    int* gsRows = nullptr;                 // n (device)
    std::vector<int> gsOffsets;            // colours + 1 (host: a sweep is one launch per colour)
    std::vector<int> gsColourOf;           // n (host): what MgLevelCopyColours hands out
    // K-cycle (MgSetCycle(mg, 1, inner)), every level that has a finer level and a map of its own -- the C of a K step: four vectors of n rows
    // and the partial sums of the step's five sums.  All null in V mode.
    double *kSpare = nullptr;              // the second cycle's other iterate buffer: c1 stays where the first cycle left it, in xa or xb
    double *kv1 = nullptr, *kv2 = nullptr, *krr = nullptr;   // A c1, A c2, b - a1 v1
    double* kPartials = nullptr;           // kKcycleSums regions of kMaxGrid doubles
    // MgUpdateValues, all null before its first call.  A level that has a map: the source list of the product that forms the next level
    // (kernels_refresh.hip).  Every level: the buffers the next refresh writes -- D^-1 and, below the first level, the values -- which change
    // places with dinv and elements when a refresh succeeds.
    int* refreshSegments = nullptr;        // nnz of the next level + 1
    int* refreshSources = nullptr;         // refreshCount stored positions of this level
    long long refreshCount = 0;
    double* shadowElements = nullptr;      // nnz (levels >= 1)
    double* shadowDinv = nullptr;          // n
};

// Multicolour ILU(0) (MgSetupIlu0): the factor of B = P (A + shift diag(A)) P^T in the colour order, rows sorted by new column.  The rows
// of colour c are the new rows [colourOffsets[c], colourOffsets[c + 1]).  y and t of the two passes are lv[0].xa and lv[0].xb.
struct MgIlu {
    double* values = nullptr; int* columns = nullptr; int* offsets = nullptr;   // nnz, nnz, n + 1 (device)
    int* diag = nullptr;                   // n: where every row's diagonal stands
    double* pinv = nullptr;                // n: 1 / pivot
    int* rowOf = nullptr;                  // n: new row -> row of A
    std::vector<int> colourOffsets;        // colours + 1 (host: a pass is one launch per colour)
    long long nnz = 0;
    int lanes = 8;                         // lanes per row of the kernels
    double pivotMin = 0.0, pivotMax = 0.0;
    double setupMs[3] = { 0.0, 0.0, 0.0 };  // checks and colouring, building B, factorisation (host clock around the phases' own synchronisations)
};

} // namespace mgcg

struct MgcgMg {
    int levels = 0;
    double omega = 0; int nu = 1, nuCoarse = 4; double sigma = 0.5;
    int interp = 0;                        // 0: piecewise-constant P (slab-local), 1: cell-centred linear P (MgSetInterpolation)
    int smoother = 0;                      // 0: weighted Jacobi, 1: multicolour Gauss-Seidel (MgSetSmoother; aggregation hierarchies only)
    int cycle = 0, cycleInner = 0;         // MgSetCycle: 0 the V-cycle, 1 the K-cycle with conjugate (0) or minimal-residual (1) inner steps; aggregation hierarchies only
    std::vector<mgcg::MgLevel> lv;
    mgcg::SpmvConfig cfg;
    hipStream_t stream = nullptr;
    MgcgComm* comm = nullptr;              // not owned
    int nranks = 1;
    bool multi = false;                    // several ranks (or one rank forced onto that path, comm_multi): full-length iterates, halo exchanges, all-reduces
    bool haloOnSide = false;               // overlap schedule (tuning knob halo_stream, resolved at set-up)
    // r.z of the PCG loop rides on the V-cycle's last sweep (single rank): partial sums go here, fusedDotCount of them
    double* fuseDotPartials = nullptr;
    int fusedDotCount = 0;
    // several ranks: the last sweep of the cycle writes the rank's rows of z = M^-1 r straight into the caller's vector (nobody needs the
    // halo of the final iterate) instead of into a full-length buffer that is then copied out
    double* finalOut = nullptr;
    bool finalWritten = false;
    bool deep = false;                     // every level >= 1 has its deep halo (decided at set-up, the same on every rank)
    bool deep0 = false;                    // ... and the finest level may form its first iterate per gather from the EXCHANGED right-hand side: every rank's
                                           // rows have one and the same diagonal and take the row-tile kernel (agreed at set-up: it decides WHAT the level exchanges)
    // deep-halo cycle, finest level: the PCG loop keeps its residual r (the cycle's right-hand side) in this buffer -- the slab's rows with
    // room for one grid plane either side -- so that ONE exchange brings r's halo planes and every sweep of the level can form its iterate
    // per gather, exactly as the single-rank cycle does (no stored first sweep, no boundary zones, no separate boundary launches)
    double* rExt = nullptr;                // plane + n + plane doubles; the loop's r = rExt + plane
    bool deepFolds = false;                // levels >= 1 form x_1 and x_1 + P e per gather too (uniform diagonals, power-of-two nx and ny)
    bool skipHalo = false;                 // the next SpMV-shaped pass finds its halo planes already in place (deep-halo cycle: formed locally)
    bool algebraic = false;                // built from aggregates of the matrix graph, not from a grid (also when it has a single level)
    int strength = 0;                      // what the matching read (MgSetupAggregationEx): 0 the level's own matrix, 1 its symmetric part
    mgcg::MgIlu* ilu = nullptr;            // MgSetupIlu0: the handle is an ILU(0) factor (one level, one rank), M^-1 = U^-1 L^-1; owned
    // MgUpdateValues (aggregation hierarchies): the handle whose analysis cache serves the levels (not owned); after the first call the
    // device flags (two ints a level: the bad row, D^-1 differs) and first D^-1 of every level that one copy brings to the host, and the
    // device bytes of the lists and shadow buffers
    MgcgSparse* sparse = nullptr;
    int* refreshFlags = nullptr; double* refreshScalars = nullptr;
    long long refreshBytes = 0;
};

namespace mgcg {

static SpmvConfig cfg_of(const MgcgSparse* h)
{
    SpmvConfig c; c.kernel = h->kernel; c.rowsPerBlock = h->rowsPerBlock; c.flags = h->flags; c.gridBlocks = h->gridBlocks; c.periodRows = h->periodRows; c.tileRows = h->tileRows; c.tilePlanes = h->tilePlanes;
    return c;
}

// the K step's vectors of one level (MgSetCycle): freed on the way back to V mode and by MgDestroy
static void kcycle_free(MgLevel& L)
{
    for (double** p : { &L.kSpare, &L.kv1, &L.kv2, &L.krr, &L.kPartials }) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

// The interior rows of a row slice -- rows [*i0, *i1) reference local columns only -- and whether its halo exchange should hide behind them
// (*active).  The range is found for every slice of several ranks (the multigrid's folded residual pass uses it with or without overlap);
// MGCG_OVERLAP decides *active: 0 never; 2 whenever an interior exists (tests); 1 (default) BY MEASUREMENT -- on slices of at least
// kOverlapMinRows rows per rank on average the plan's own exchange is timed in line against the fork / launch / join round trip of the
// overlap schedule on this communicator (halo_overlap_pays, comm.hip: once per plan, the same answer on every rank), and the exchange is
// hidden only where it costs more than the hops that hide it.  (Round 3 decided by size alone, >= 3 M rows: on the one-rank RCCL
// communicator of a one-GPU box that rule picked the slowest schedule measured, profiles/r3/slab_latency_box_e_final_code.json.)
// halo / vec: the plan of the slice and the full-length vector it exchanges.  nGlobal: rows of all ranks (the same number everywhere,
// so all ranks enter the measurement's collective together or not at all).
// d2: two device ints of the caller's workspace (Workspace::devInts + 6)
constexpr long long kOverlapMinRows = 1000000;
static bool plan_overlap(hipStream_t s, MgcgComm* comm, bool multi, const int* rowOffsets, const int* columnIndeces,
                         long long n, long long offset, bool* active, long long* i0, long long* i1, int* d2,
                         HaloPlan* halo, double* vec, long long nGlobal)
{
    *active = false; *i0 = 0; *i1 = 0;
    halo_overlap_clear_times();                     // MgcgLastOverlapTimes speaks of the last plan: nothing measured yet
    if (!multi) return true;
    const int mode = tuning().overlap.load(std::memory_order_relaxed);
    bool wanted = mode == 2;
    if (mode == 1 && nGlobal >= kOverlapMinRows * (long long)MgcgCommSize(comm)) {
        if (!halo_overlap_pays(comm, halo, vec, s, &wanted)) return false;       // collective
    }
    if (n <= 0) return true;
    if (MgcgCommSize(comm) == 1) {
        // one rank forced onto the several-ranks path (measurement): an artificial split -- the first and last force_multirank rows
        // (rounded to SpMV tiles) play the boundary
        long long w = tuning().forceMultiRank.load(std::memory_order_relaxed);
        w = (w + 255) & ~255LL;
        if (n >= 4 * w && w > 0) { *i0 = w; *i1 = n - w; *active = wanted && halo_overlap_available(comm); }
        return true;
    }
    int h2[2] = { 0, (int)n };
    bool ok = MGCG_HIP(hipMemcpyAsync(d2, h2, sizeof(h2), hipMemcpyHostToDevice, s));
    if (ok) launch_halo_rows(s, rowOffsets, columnIndeces, n, offset, d2);
    ok = ok && MGCG_HIP(hipMemcpyAsync(h2, d2, sizeof(h2), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (!ok) return false;
    const long long lo = h2[0], hi = h2[1] < n ? h2[1] : n;
    if (hi > lo) {
        *i0 = lo; *i1 = hi;
        *active = wanted && (mode == 2 || 2 * (hi - lo) >= n) && halo_overlap_available(comm);
    }
    return true;
}

static bool mg_halo(MgcgMg* mg, MgLevel& L, double* xfull)
{
    if (!mg->multi || mg->skipHalo) return true;
    return halo_exchange(mg->comm, L.halo, xfull, mg->stream);
}

// Halo of the full-length iterate xfull, then the SpMV-shaped pass; interior rows first when the level overlaps.
// partials / nPartials (dot epilogues): where the per-workgroup partial sums go and how many were written.
// aInt describes the pass for the interior rows (they reference local columns only), aBnd for the boundary rows and for a level that
// does not overlap: the same arguments except, for the folded residual pass of several ranks (mg_vcycle), the multiplied vector.
static bool mg_spmv2(MgcgMg* mg, MgLevel& L, int epilogue, const SpmvArgs& aInt, const SpmvArgs& aBnd, double* xfull, double* partials = nullptr, int* nPartials = nullptr,
                     bool splitInLine = false)
{
    hipStream_t s = mg->stream;
    int n = 0;
    if (nPartials) *nPartials = 0;
    const int half = partials ? kMaxPartials / 2 : 0;
    if (!L.overlap || mg->skipHalo) {                  // (nothing travels: nothing to hide)
        if (!mg_halo(mg, L, xfull)) return false;
        if (splitInLine) {                           // two kinds of rows, one stream: interior rows with aInt, the rows either side with aBnd
            n = launch_spmv_range(s, epilogue, aInt, L.cfg, L.dcsr, L.interior0, L.interior1, partials, half);
            n += launch_spmv_two_ranges(s, epilogue, aBnd, L.cfg, L.dcsr, L.interior0, L.interior1, partials ? partials + n : nullptr, half);
        } else {
            SpmvArgs b = aBnd; b.partials = partials;
            n = launch_spmv_auto(s, epilogue, b, L.cfg, L.dcsr);
        }
        if (nPartials) *nPartials = n;
        return true;
    }
    hipStream_t side = halo_overlap_fork(mg->comm, s);
    if (!side) return false;
    if (mg->haloOnSide) {
        // the exchange on the side stream, all rows on the main stream: both cross-stream hops hide behind the interior rows
        if (!halo_exchange(mg->comm, L.halo, xfull, side)) return false;
        n = launch_spmv_range(s, epilogue, aInt, L.cfg, L.dcsr, L.interior0, L.interior1, partials, half);
        if (!halo_overlap_join(mg->comm, s)) return false;
        n += launch_spmv_two_ranges(s, epilogue, aBnd, L.cfg, L.dcsr, L.interior0, L.interior1, partials ? partials + n : nullptr, half);   // the boundary rows either side of the interior
        if (nPartials) *nPartials = n;
        return true;
    }
    n = launch_spmv_range(side, epilogue, aInt, L.cfg, L.dcsr, L.interior0, L.interior1, partials, half);
    if (!mg_halo(mg, L, xfull)) return false;
    n += launch_spmv_two_ranges(s, epilogue, aBnd, L.cfg, L.dcsr, L.interior0, L.interior1, partials ? partials + n : nullptr, half);
    if (nPartials) *nPartials = n;
    return halo_overlap_join(mg->comm, s);
}
static bool mg_spmv(MgcgMg* mg, MgLevel& L, int epilogue, const SpmvArgs& a, double* xfull, double* partials = nullptr, int* nPartials = nullptr)
{
    return mg_spmv2(mg, L, epilogue, a, a, xfull, partials, nPartials);
}

// xout_loc = xin_loc + omega * (dinv * (b - A xin)); xin / xout are full-length buffers
constexpr long long kFoldUpMaxRows = 100000000;     // (bench.py FOLD_UP_MAX_ROWS counts the bytes with the same limit)
static thread_local int t_lastFolds = 0;        // MgcgLastVcycleFolds: bit 0 first sweep folded, bit 1 prolongation folded (last V-cycle of this thread)

static int log2_exact(long long v) { int l = 0; while ((1LL << l) < v) ++l; return ((1LL << l) == v) ? l : -1; }

// coarse != nullptr (one rank, V(1,1), uniform diagonal, row-tile kernel on plain CSR, power-of-two nx and ny): the sweep runs on
// x1 + P e without that iterate ever being stored -- x1 = omega (d0 b) and the parent's correction are formed per gather and for the
// row itself (SpmvArgs::xScaled == 2); xin is not read.
// Several ranks (coarse = the FULL-length coarse iterate, interiorOnly): only the interior rows form it on the fly (their columns are
// local: (b - offset)[col]); the boundary rows multiply the stored iterate, which the caller has written within two planes of the
// rank's boundaries and mg_spmv2 exchanges.
// globalB (deep-halo cycle, b has its halo planes): ALL rows of the rank form the iterate per gather -- b is addressed by global column ids
// ((b - offset)[col]) and coarse is the full-length coarse result; one launch, as on a single rank.
static bool mg_jacobi(MgcgMg* mg, MgLevel& L, const double* b, double* xin, double* xout, const int* done, bool withDot = false, const double* coarse = nullptr,
                      bool interiorOnly = false, bool globalB = false)
{
    SpmvArgs a{};
    a.elements = L.elements; a.rowOffsets = L.rowOffsets; a.columnIndeces = L.columnIndeces; a.x = xin; a.y = xout + L.offset;
    a.elementsCount = (int)L.nnz; a.rowCount = (int)L.n; a.columnCount = (int)L.nGlobal;
    a.w = xin + L.offset; a.b = b; a.dinv = L.dinv; a.dinvUniform = L.dinvUniform ? 1 : 0; a.dinvScalar = L.dinvScalar; a.omega = mg->omega; a.doneFlag = done;
    SpmvArgs stored = a;                            // (the sweep on a stored iterate: what the boundary rows of several ranks run)
    if (coarse != nullptr) {
        const int lx = log2_exact(L.nx), ly = log2_exact(L.ny);
        a.x = b - ((interiorOnly || globalB) ? L.offset : 0); a.w = nullptr; a.xScaled = 2; a.xInner = L.dinvScalar; a.xOuter = mg->omega; a.xCoarse = coarse;
        const int sy = L.ny > 1 ? 1 : 0, sz = L.nz > 1 ? 1 : 0;
        a.cM0 = L.nx / 2 - 1; a.cS1 = 1 + sy; a.cM1 = ((L.ny >> sy) - 1) << (lx - 1);
        a.cS2 = 1 + sy + sz; a.cM2 = (int)(~0u << (lx - 1 + ly - sy));
        a.cRowBase = (interiorOnly || globalB) ? (int)L.offset : 0;
    }
    if (interiorOnly) {
        if (withDot && mg->finalOut != nullptr) { a.y = mg->finalOut; stored.y = mg->finalOut; mg->finalWritten = true; }
        const bool dot = withDot && mg->fuseDotPartials != nullptr;
        return mg_spmv2(mg, L, dot ? EPI_JACOBI_DOT : EPI_JACOBI, a, stored, xin, dot ? mg->fuseDotPartials : nullptr, dot ? &mg->fusedDotCount : nullptr, true);
    }
    // withDot marks the LAST sweep of the cycle on the finest level: r.z of the PCG loop rides on it (partial sums of b . xout), and
    // with several ranks it writes the rank's rows of the result where the caller wants them
    if (withDot && mg->multi && mg->finalOut != nullptr) { a.y = mg->finalOut; mg->finalWritten = true; }
    if (withDot && mg->fuseDotPartials != nullptr) {
        if (!mg->multi) {
            a.partials = mg->fuseDotPartials;
            mg->fusedDotCount = launch_spmv_auto(mg->stream, EPI_JACOBI_DOT, a, L.cfg, L.dcsr);
            return true;
        }
        return mg_spmv(mg, L, EPI_JACOBI_DOT, a, xin, mg->fuseDotPartials, &mg->fusedDotCount);
    }
    return mg_spmv(mg, L, EPI_JACOBI, a, xin);
}

// `sweeps` Jacobi sweeps on level L for right-hand side b.  first: the first sweep starts from zero.
// cur is the buffer holding the iterate (ignored when first); *result receives the buffer holding the result.
// Under MgSetSmoother(mg, 1) the sweeps are multicolour Gauss-Seidel sweeps in place on cur (other is not touched): one launch per colour on
// the level's plain CSR.  The last level alternates forward (colours 0, 1, ...) and backward sweeps from a forward one; a level with a map
// sweeps forward before the coarse correction (first) and backward after it.  A first sweep starts from +0.0 stored by a pass of its own.
// dotOnLast is not served here: the cycle reports no partial sums and the loop runs its own r.z pass (mg_apply: *nDot = 0).
static bool mg_smooth(MgcgMg* mg, MgLevel& L, const double* b, double* cur, double* other, int sweeps, bool first, const int* done, double** result,
                      bool dotOnLast = false)
{
    if (mg->smoother == 1) {
        const bool last = &L == &mg->lv[(size_t)mg->levels - 1];
        const int colours = (int)L.gsOffsets.size() - 1;
        const double avgRow = L.n > 0 ? (double)L.nnz / (double)L.n : 0.0;
        if (first) launch_gs_zero(mg->stream, L.n, cur, done);
        for (int sIdx = 0; sIdx < sweeps; ++sIdx) {
            const bool forward = last ? (sIdx % 2 == 0) : first;
            for (int q = 0; q < colours; ++q) {
                const int c = forward ? q : colours - 1 - q;
                launch_gs_sweep(mg->stream, L.gsRows + L.gsOffsets[(size_t)c], L.gsOffsets[(size_t)c + 1] - L.gsOffsets[(size_t)c], L.elements, L.rowOffsets,
                                L.columnIndeces, b, L.dinv, mg->omega, cur, avgRow, done);
            }
        }
        *result = cur;
        return true;
    }
    for (int sIdx = 0; sIdx < sweeps; ++sIdx) {
        if (first && sIdx == 0) {
            launch_jacobi_first(mg->stream, L.n, mg->omega, L.dinv, L.dinvUniform ? 1 : 0, L.dinvScalar, b, cur + L.offset, done);
        } else {
            if (!mg_jacobi(mg, L, b, cur, other, done, dotOnLast && sIdx == sweeps - 1)) return false;
            double* t = cur; cur = other; other = t;
        }
    }
    *result = cur;
    return true;
}

// ---------------------------------------------------------------- deep-halo cycle (several ranks, V(1,1), piecewise-constant transfer)
// The per-sweep schedule above exchanges a halo plane before EVERY SpMV-shaped pass: on 3 levels with 4 coarse sweeps that is seven exchanges
// per cycle (two on the finest level, two on the middle one, three on the coarsest), each a latency-bound grouped send/recv -- where the
// reference's loop has ONE exchange per iteration (SyncP, ConjugateGradientParallelGpu.cs:384-419,469).  Here every level >= 1 takes ONE
// exchange per cycle: `deep` planes of its RIGHT-HAND SIDE either side of the slab, after which everything the level computes within reach
// of its boundaries is recomputed locally on those planes -- the same operations on the same values in the same order, so every entry is the
// bit the owning rank computes (tests: z = M^-1 r equal to the single-domain oracle bit for bit).  Counting planes of the level:
//   coarsest level, nu_c sweeps, result wanted one plane beyond the slab (the finer level prolongs it onto ITS halo planes):
//     x_1 = omega D^-1 b on +-nu_c planes, sweep k on +-(nu_c + 1 - k), x_{nu_c} on +-1          -> deep = nu_c
//   a middle level: x_1 = omega D^-1 b on +-2, residual on the slab, y = x_1 + P e on +-2 (e from below on +-1 of ITS planes = +-2 of these),
//     post-smoothing sweep on +-1                                                              -> deep = 2
//   the finest level has one exchange too: of its right-hand side when that is the loop's r in MgcgMg::rExt and every rank holds the same
//     uniform diagonal (MgcgMg::deep0, agreed at set-up: x_1 and x_1 + P e are then formed per gather on all rows), else of the stored x_1
//     before the residual pass -- the post-smoothing sweep then finds x_1 in the halo planes and P e is added there (mg_deep_prolong_halo);
//     either way                                                                                       -> no second exchange.
// Per MGCG iteration: SyncP of p + 3 exchanges in the cycle instead of SyncP + 7.  The redundant rows are deep planes on slabs of 32 / 16
// planes of levels that hold 1/8 and 1/64 of the work.
static bool mg_deep_level(MgcgMg* mg, int l, const int* done, double** result)
{
    MgLevel& L = mg->lv[l];
    hipStream_t s = mg->stream;
    const long long plane = (long long)L.nx * L.ny;
    const bool coarsest = l == mg->levels - 1;
    auto zlo = [&](int d) { const int z = L.z0 - d; return z < L.extZ0 ? L.extZ0 : z; };
    auto zhi = [&](int d) { const int z = L.z1 + d; return z > L.extZ1 ? L.extZ1 : z; };
    // rows of planes [za, zb) of the extended slab
    auto first = [&](int d, double* x) {            // x = omega D^-1 b on +-d planes
        const long long r0 = (long long)zlo(d) * plane, r1 = (long long)zhi(d) * plane;
        launch_jacobi_first(s, r1 - r0, mg->omega, L.extDinv + (r0 - L.extBase), 0, 0.0, L.bFull + r0, x + r0, done);
    };
    auto sweep = [&](int d, double* xin, double* xout) {   // xout = xin + omega D^-1 (b - A xin) on +-d planes
        const long long r0 = (long long)zlo(d) * plane - L.extBase, r1 = (long long)zhi(d) * plane - L.extBase;
        SpmvArgs a{};
        a.elements = L.extElements; a.rowOffsets = L.extRowOffsets; a.columnIndeces = L.extColumnIndeces; a.x = xin; a.y = xout + L.extBase;
        a.elementsCount = (int)L.extNnz; a.rowCount = (int)L.extRows; a.columnCount = (int)L.nGlobal;
        a.w = xin + L.extBase; a.b = L.bFull + L.extBase; a.dinv = L.extDinv; a.dinvUniform = 0; a.omega = mg->omega; a.doneFlag = done;
        (void)launch_spmv_range(s, EPI_JACOBI, a, L.cfg, nullptr, r0, r1, nullptr, 0);
    };
    if (!halo_exchange(mg->comm, L.bHalo, L.bFull, s)) return false;                  // the level's ONE exchange
    if (coarsest) {
        double* cur = L.xa; double* other = L.xb;
        first(mg->nuCoarse, cur);
        for (int k = 2; k <= mg->nuCoarse; ++k) { sweep(mg->nuCoarse + 1 - k, cur, other); double* t = cur; cur = other; other = t; }
        *result = cur;                                                               // valid on the slab and one plane either side
        return true;
    }
    MgLevel& C = mg->lv[l + 1];
    const bool folded = mg->deepFolds && (L.dcsr == nullptr || !L.dcsr->usable) &&   // (a compact form of the level's own matrix keeps the stored iterates)
                        tuning().noFold.load(std::memory_order_relaxed) == 0 && tuning().foldUp.load(std::memory_order_relaxed) != 0;
    if (!folded) first(2, L.xa);
    SpmvArgs a{};                                                                    // r = b - A x_1 on the slab (the level's own matrix)
    a.elements = L.elements; a.rowOffsets = L.rowOffsets; a.columnIndeces = L.columnIndeces; a.x = L.xa; a.y = L.r;
    a.elementsCount = (int)L.nnz; a.rowCount = (int)L.n; a.columnCount = (int)L.nGlobal; a.b = L.b; a.doneFlag = done;
    if (folded) { a.x = L.bFull; a.xScaled = 1; a.xInner = L.dinvScalar; a.xOuter = mg->omega; }   // x_1[col] = omega (d0 b[col]) per gather: b is full length
    (void)launch_spmv_auto(s, EPI_RESIDUAL, a, L.cfg, L.dcsr);
    launch_restrict(s, L.nx, L.ny, L.z1 - L.z0, L.r, C.b, done);                      // b_c = P^T r (slab-local)
    double* e = nullptr;
    if (!mg_deep_level(mg, l + 1, done, &e)) return false;
    if (folded) {
        // post-smoothing sweep on +-1 plane with x_1 + P e formed per gather (and for the row itself): b on +-2 and e on +-1 coarse plane are here
        const long long r0 = (long long)zlo(1) * plane - L.extBase, r1 = (long long)zhi(1) * plane - L.extBase;
        SpmvArgs f{};
        f.elements = L.extElements; f.rowOffsets = L.extRowOffsets; f.columnIndeces = L.extColumnIndeces; f.x = L.bFull; f.y = L.xb + L.extBase;
        f.elementsCount = (int)L.extNnz; f.rowCount = (int)L.extRows; f.columnCount = (int)L.nGlobal;
        f.w = nullptr; f.b = L.bFull + L.extBase; f.dinv = L.extDinv; f.dinvUniform = 1; f.dinvScalar = L.dinvScalar; f.omega = mg->omega; f.doneFlag = done;
        f.xScaled = 2; f.xInner = L.dinvScalar; f.xOuter = mg->omega; f.xCoarse = e;
        const int lx = log2_exact(L.nx), ly = log2_exact(L.ny), sy = L.ny > 1 ? 1 : 0, sz = L.nz > 1 ? 1 : 0;
        f.cM0 = L.nx / 2 - 1; f.cS1 = 1 + sy; f.cM1 = ((L.ny >> sy) - 1) << (lx - 1);
        f.cS2 = 1 + sy + sz; f.cM2 = (int)(~0u << (lx - 1 + ly - sy));
        f.cRowBase = (int)L.extBase;
        (void)launch_spmv_range(s, EPI_JACOBI, f, L.cfg, nullptr, r0, r1, nullptr, 0);
        *result = L.xb;
        return true;
    }
    const int za = zlo(2), zb = zhi(2);                                              // (even planes: the slab is aligned and 2 is even)
    launch_prolong_add(s, L.nx, L.ny, zb - za, L.xa + (long long)za * plane, e + (long long)(za / 2) * C.nx * C.ny, done);   // y = x_1 + P e on +-2
    sweep(1, L.xa, L.xb);
    *result = L.xb;                                                                  // valid on the slab and one plane either side
    return true;
}

// the finest level's halo planes of `cur` hold x_1 (from the exchange before the residual pass): add P e there, so that the post-smoothing
// sweep needs no exchange.  e: the coarse result, valid one coarse plane beyond the slab.
static void mg_deep_prolong_halo(MgcgMg* mg, MgLevel& L, MgLevel& C, double* cur, const double* e, const int* done)
{
    const long long plane = (long long)L.nx * L.ny, cplane = (long long)C.nx * C.ny;
    if (L.z0 > 0) launch_prolong_add(mg->stream, L.nx, L.ny, 1, cur + (long long)(L.z0 - 1) * plane, e + (long long)((L.z0 - 1) / 2) * cplane, done);
    if (L.z1 < L.nz) launch_prolong_add(mg->stream, L.nx, L.ny, 1, cur + (long long)L.z1 * plane, e + (long long)(L.z1 / 2) * cplane, done);
}

static bool mg_vcycle(MgcgMg* mg, int l, const double* b, double* x0, double* x1, const int* done, double** result);

// The K step on level c of an aggregation hierarchy in K mode (MgSetCycle; the contract is written out in include/MgcgGpu.h), in place of
// one cycle for the level's right-hand side C.b: two Krylov steps preconditioned by the cycle.  c1 stays in the iterate buffer the first
// cycle leaves it in; the second cycle ping-pongs between the other one and kSpare.  *result receives e, formed in c2's buffer.  The
// launch sequence does not depend on the data: a breakdown is decided inside the passes (kernels_kcycle.hip).
static bool mg_kstep(MgcgMg* mg, int c, const int* done, double** result)
{
    MgLevel& C = mg->lv[c];
    hipStream_t s = mg->stream;
    auto product = [&](double* x, double* y) {               // y = A_C x: the level's own product, rows summed as every pass of the level sums them
        SpmvArgs a{};
        a.elements = C.elements; a.rowOffsets = C.rowOffsets; a.columnIndeces = C.columnIndeces; a.x = x; a.y = y;
        a.elementsCount = (int)C.nnz; a.rowCount = (int)C.n; a.columnCount = (int)C.nGlobal; a.alpha = 1.0; a.beta = 0.0; a.doneFlag = done;
        return mg_spmv(mg, C, EPI_AXPBY, a, x);
    };
    double *c1 = nullptr, *c2 = nullptr;
    if (!mg_vcycle(mg, c, C.b, C.xa, C.xb, done, &c1) || !product(c1, C.kv1)) return false;
    int nSums = launch_kcycle_sums1(s, mg->cycleInner, c1, C.kv1, C.b, C.n, C.kPartials, done);
    launch_kcycle_residual(s, C.b, C.kv1, C.krr, C.n, C.kPartials, nSums, done);
    if (!mg_vcycle(mg, c, C.krr, c1 == C.xa ? C.xb : C.xa, C.kSpare, done, &c2) || !product(c2, C.kv2)) return false;
    nSums = launch_kcycle_sums2(s, mg->cycleInner, c2, C.kv2, C.kv1, C.krr, C.n, C.kPartials, done);
    launch_kcycle_combine(s, c1, c2, c2, C.n, C.kPartials, nSums, done);
    *result = c2;
    return true;
}

// One V(nu,nu) cycle on level l for right-hand side b (local); x0/x1 are that level's two full-length iterate
// buffers.  *result receives the buffer that holds the answer.  Mirrors vcycle() of oracle/mg_oracle.c.
static bool mg_vcycle(MgcgMg* mg, int l, const double* b, double* x0, double* x1, const int* done, double** result)
{
    MgLevel& L = mg->lv[l];
    if (l == mg->levels - 1) return mg_smooth(mg, L, b, x0, x1, mg->nuCoarse, true, done, result, l == 0);
    MgLevel& C = mg->lv[l + 1];
    double* cur = nullptr;
    if (L.agg != nullptr) {
        // a level of an aggregation hierarchy: the stored cycle with the indexed transfer (the folded forms address parents by bit fields
        // of grid indices).  One rank: nothing travels.
        if (!mg_smooth(mg, L, b, x0, x1, mg->nu, true, done, &cur)) return false;
        double* spare = (cur == x0) ? x1 : x0;
        SpmvArgs ar{};
        ar.elements = L.elements; ar.rowOffsets = L.rowOffsets; ar.columnIndeces = L.columnIndeces; ar.x = cur; ar.y = L.r;
        ar.elementsCount = (int)L.nnz; ar.rowCount = (int)L.n; ar.columnCount = (int)L.nGlobal; ar.b = b; ar.doneFlag = done;
        if (!mg_spmv(mg, L, EPI_RESIDUAL, ar, cur)) return false;                              // r = b - A x
        launch_amg_restrict(mg->stream, C.n, L.aggOffsets, L.aggMembers, L.r, C.b, done);      // b_c = P^T r
        double* ec = nullptr;
        if (C.kSpare != nullptr ? !mg_kstep(mg, l + 1, done, &ec) : !mg_vcycle(mg, l + 1, C.b, C.xa, C.xb, done, &ec)) return false;   // (K mode, and C has a map of its own)
        launch_amg_prolong_add(mg->stream, L.n, L.agg, cur, ec, done);                         // x += P e
        return mg_smooth(mg, L, b, cur, spare, mg->nu, false, done, result, l == 0);
    }
    // V(1,*) on one rank with a uniform diagonal: the first sweep x1 = omega (d0 b) is not stored; the residual pass forms x1[col] per
    // gather (row-pattern form, or the row-tile kernel on plain CSR) and the prolongation forms x1[i] again when it adds the correction
    const bool linear = mg->interp == 1;
    bool canScale = false;
    if (L.dcsr != nullptr && L.dcsr->usable) canScale = L.dcsr->patternId != nullptr;
    else {
        SpmvArgs probe{}; probe.elements = L.elements; probe.columnIndeces = L.columnIndeces; probe.elementsCount = (int)L.nnz; probe.rowCount = (int)L.n;
        canScale = spmv_takes_rowtile(probe, L.cfg);
    }
    const bool mayFold = mg->nu == 1 && !linear && L.dinvUniform && canScale && tuning().noFold.load(std::memory_order_relaxed) == 0;
    const bool fold = mayFold && !mg->multi;
    // Deep-halo cycle with the right-hand side in the loop's extended buffer (b = rExt + plane: one grid plane of room either side): ONE
    // exchange brings b's halo planes, after which every row of the rank -- boundary rows included -- forms x_1 per gather of the residual
    // pass and x_1 + P e per gather of the post-smoothing sweep: the single-rank cycle's kernels, one launch each, no zones.
    if (l == 0 && mg->deep && mg->deep0 && mg->rExt != nullptr && b == mg->rExt + (long long)L.nx * L.ny && mayFold && (L.dcsr == nullptr || !L.dcsr->usable) &&
        L.nx >= 2 && log2_exact(L.nx) >= 1 && log2_exact(L.ny) >= 0 && L.nGlobal < 0x7fffffffLL && tuning().foldUp.load(std::memory_order_relaxed) != 0) {
        SpmvArgs a{};
        a.elements = L.elements; a.rowOffsets = L.rowOffsets; a.columnIndeces = L.columnIndeces; a.x = b - L.offset; a.y = L.r;
        a.elementsCount = (int)L.nnz; a.rowCount = (int)L.n; a.columnCount = (int)L.nGlobal; a.b = b; a.doneFlag = done;
        a.xScaled = 1; a.xInner = L.dinvScalar; a.xOuter = mg->omega;
        if (!mg_spmv(mg, L, EPI_RESIDUAL, a, const_cast<double*>(b) - L.offset)) return false;     // the level's one exchange (b's halo planes), then r = b - A x_1
        launch_restrict(mg->stream, L.nx, L.ny, L.z1 - L.z0, L.r, C.b, done);
        double* e = nullptr;
        if (!mg_deep_level(mg, 1, done, &e)) return false;
        t_lastFolds |= 1 | 2 | 4 | 8;
        struct SkipHalo { MgcgMg* m; ~SkipHalo() { m->skipHalo = false; } } skip{ mg };
        mg->skipHalo = true;
        if (!mg_jacobi(mg, L, b, x0, x1, done, true, e, false, true)) return false;              // the last sweep (+ r.z), straight into the caller's z
        *result = x1;
        return true;
    }
    // Several ranks: the same fold for the INTERIOR rows (they reference local columns only: x1[col] formed per gather
    // from the local right-hand side), while the boundary rows multiply the stored iterate, which therefore exists only where they reach --
    // the local rows within two grid planes of a boundary (every level is a 27-point-neighbourhood operator: MgSetup's Galerkin pass has
    // checked it) -- and, after the exchange, in the halo planes.
    const long long plane = (long long)L.nx * L.ny;
    const long long zoneLo = L.interior0 > 0 ? L.interior0 + 2 * plane : 0;                 // x1 stored for local rows [0, zoneLo) ...
    const long long zoneHi = L.interior1 < L.n ? L.interior1 - 2 * plane : L.n;             // ... and [zoneHi, n)
    // (worth two more launches only on a large level: 16 bytes per row saved against ~15 us of launches and a boundary pass of its own)
    const bool foldInterior = mayFold && mg->multi && (L.dcsr == nullptr || !L.dcsr->usable) && zoneLo <= zoneHi && 2 * (L.interior1 - L.interior0) >= L.n &&
                              (L.n >= 3000000 || tuning().overlap.load(std::memory_order_relaxed) == 2);
    if (fold || foldInterior) t_lastFolds |= 1;
    if (fold) cur = x0;
    else if (foldInterior) {
        cur = x0;
        if (zoneLo > 0) launch_jacobi_first(mg->stream, zoneLo, mg->omega, L.dinv, 1, L.dinvScalar, b, cur + L.offset, done);
        if (zoneHi < L.n) launch_jacobi_first(mg->stream, L.n - zoneHi, mg->omega, L.dinv, 1, L.dinvScalar, b + zoneHi, cur + L.offset + zoneHi, done);
    }
    else if (!mg_smooth(mg, L, b, x0, x1, mg->nu, true, done, &cur)) return false;
    double* other = (cur == x0) ? x1 : x0;
    SpmvArgs a{};
    // linear transfer on several ranks: the restriction reads one plane of r from each z-neighbour, so r goes to the spare
    // full-length iterate buffer (dead until the post-smoothing writes it) and that plane is exchanged
    const bool rFullLength = linear && mg->multi;
    a.elements = L.elements; a.rowOffsets = L.rowOffsets; a.columnIndeces = L.columnIndeces; a.x = fold ? b : cur; a.y = rFullLength ? other + L.offset : L.r;
    a.elementsCount = (int)L.nnz; a.rowCount = (int)L.n; a.columnCount = (int)L.nGlobal; a.b = b; a.doneFlag = done;
    if (fold) { a.xScaled = 1; a.xInner = L.dinvScalar; a.xOuter = mg->omega; }
    if (foldInterior) {
        SpmvArgs ai = a;
        ai.x = b - L.offset;                         // global column ids of the interior rows are local: (b - offset)[col] = b[col - offset]
        ai.xScaled = 1; ai.xInner = L.dinvScalar; ai.xOuter = mg->omega;
        if (!mg_spmv2(mg, L, EPI_RESIDUAL, ai, a, cur, nullptr, nullptr, true)) return false;   // r = b - A x1, interior rows from b, boundary rows from the exchanged iterate
    }
    else if (!mg_spmv(mg, L, EPI_RESIDUAL, a, cur)) return false;                             // r = b - A x
    if (linear) {
        if (rFullLength && !halo_exchange(mg->comm, L.transferHalo, other, mg->stream)) return false;
        launch_restrict_linear(mg->stream, L.nx, L.ny, L.nz, L.z0, L.z1, rFullLength ? other : L.r, C.b, done);   // b_c = P^T r
    } else {
        launch_restrict(mg->stream, L.nx, L.ny, L.z1 - L.z0, L.r, C.b, done);                 // b_c = P^T r (slab-local)
    }
    double* e = nullptr;
    const bool deep = mg->deep && !linear && l == 0;                                      // (levels >= 1 of a deep-halo cycle never come through here)
    if (deep) { if (!mg_deep_level(mg, 1, done, &e)) return false; t_lastFolds |= 4; }
    else if (!mg_vcycle(mg, l + 1, C.b, C.xa, C.xb, done, &e)) return false;
    // deep-halo cycle: the post-smoothing sweep's halo planes are formed here (x_1 is in them since the residual pass's exchange, P e is
    // added by mg_deep_prolong_halo), so the sweep itself exchanges nothing
    struct SkipHalo { MgcgMg* m; bool on; ~SkipHalo() { if (on) m->skipHalo = false; } } skip{ mg, deep };
    if (linear) {
        if (mg->multi && !halo_exchange(mg->comm, C.transferHalo, e, mg->stream)) return false;
        launch_prolong_linear_add(mg->stream, L.nx, L.ny, L.nz, L.z0, L.z1, cur + L.offset, e, done);               // x += P e
    }
    else if (fold && (L.dcsr == nullptr || !L.dcsr->usable) && L.nx >= 2 && log2_exact(L.nx) >= 1 && log2_exact(L.ny) >= 0 && L.nGlobal < 0x7fffffffLL &&
             (tuning().foldUp.load(std::memory_order_relaxed) < 0 ? L.n <= kFoldUpMaxRows : tuning().foldUp.load(std::memory_order_relaxed) != 0)) {
        // V(1,1) on plain CSR: the prolongation is folded into the one post-smoothing sweep as well -- x1 + P e is formed per gather there
        // (no prolongation kernel, the iterate buffer `cur` is never written: 33 N bytes less on this level).  The second gather per entry
        // costs the sweep more than the bytes save on the largest levels (profiles/r3/foldup_ab.log, the A/B script is in the history: 256^3 as the
        // finest level -4.5 % per MGCG iteration, 512 x 512 x 256 -1.6 %, as level 1 of 512^3 -56 us; on the 512^3 level itself +0.13 ms): by level size.
        if (!mg_jacobi(mg, L, b, cur, other, done, l == 0, e + C.offset)) return false;
        t_lastFolds |= 2;
        *result = other;
        return true;
    }
    else if (foldInterior && L.nx >= 2 && log2_exact(L.nx) >= 1 && log2_exact(L.ny) >= 0 && L.nGlobal < 0x7fffffffLL && L.nz > 1 && (L.z0 & 1) == 0 && ((L.z1 - L.z0) & 1) == 0 &&
             (tuning().foldUp.load(std::memory_order_relaxed) < 0 ? L.n <= kFoldUpMaxRows : tuning().foldUp.load(std::memory_order_relaxed) != 0)) {
        // several ranks: the same for the interior rows; x1 + P e is stored only where the boundary rows reach (the zones of the first fold, the
        // upper one begun on an even plane so that its parents start on a whole coarse plane), and the halo planes arrive by the exchange
        const long long planes = L.z1 - L.z0, coarsePlane = (long long)C.nx * C.ny;
        const long long loPlanes = zoneLo / plane;
        long long hiStart = zoneHi / plane;
        if (hiStart & 1) --hiStart;
        if (hiStart < loPlanes) {                                                   // the zones meet: the whole slab in one piece
            launch_prolong_scaled(mg->stream, L.nx, L.ny, (int)planes, cur + L.offset, b, L.dinvScalar, mg->omega, e + C.offset, done);
        } else {
            if (loPlanes > 0) launch_prolong_scaled(mg->stream, L.nx, L.ny, (int)loPlanes, cur + L.offset, b, L.dinvScalar, mg->omega, e + C.offset, done);
            if (zoneHi < L.n) {
                const long long r0 = hiStart * plane;
                launch_prolong_scaled(mg->stream, L.nx, L.ny, (int)(planes - hiStart), cur + L.offset + r0, b + r0, L.dinvScalar, mg->omega,
                                      e + C.offset + (hiStart / 2) * coarsePlane, done);
            }
        }
        if (deep) { mg_deep_prolong_halo(mg, L, C, cur, e, done); mg->skipHalo = true; }
        if (!mg_jacobi(mg, L, b, cur, other, done, l == 0, e, true)) return false;
        t_lastFolds |= 2;
        *result = other;
        return true;
    }
    else if (fold || foldInterior) launch_prolong_scaled(mg->stream, L.nx, L.ny, L.z1 - L.z0, cur + L.offset, b, L.dinvScalar, mg->omega, e + C.offset, done);
    else launch_prolong_add(mg->stream, L.nx, L.ny, L.z1 - L.z0, cur + L.offset, e + C.offset, done);   // x += P e (slab-local)
    if (deep) { mg_deep_prolong_halo(mg, L, C, cur, e, done); mg->skipHalo = true; }
    return mg_smooth(mg, L, b, cur, other, mg->nu, false, done, result, l == 0);
}

// z = M^-1 r (both local).  A single rank ping-pongs level 0 between z itself and lv[0].xa so that the result
// lands in z; with several ranks the iterates must be full length, so the result is copied out of lv[0].xa/xb.
// dotPartials (optional, single rank): the last sweep also leaves *nDot partial sums of r . z there (0: not fused,
// the caller runs the dot product itself).
static bool mg_apply(MgcgMg* mg, const double* r, double* z, const int* done, double* dotPartials = nullptr, int* nDot = nullptr)
{
    mg->fuseDotPartials = dotPartials; mg->fusedDotCount = 0;
    t_lastFolds = 0;
    struct Reset { MgcgMg* m; int* n; ~Reset() { if (n) *n = m->fusedDotCount; m->fuseDotPartials = nullptr; } } reset{ mg, nDot };
    MgLevel& L0 = mg->lv[0];
    if (mg->ilu != nullptr) {
        // z = U^-1 L^-1 r: forward over the colours ascending, backward descending, one launch each; no r.z is reported (*nDot = 0)
        const MgIlu& F = *mg->ilu;
        const int colours = (int)F.colourOffsets.size() - 1;
        for (int pass = 0; pass < 2; ++pass)
            for (int q = 0; q < colours; ++q) {
                const int c = pass == 0 ? q : colours - 1 - q;
                launch_ilu_pass(mg->stream, pass == 1, F.colourOffsets[(size_t)c], F.colourOffsets[(size_t)c + 1] - F.colourOffsets[(size_t)c], F.values, F.offsets,
                                F.columns, F.diag, F.pinv, F.rowOf, r, L0.xa, L0.xb, z, F.lanes, done);
            }
        return MGCG_HIP(hipGetLastError());
    }
    double* res = nullptr;
    if (!mg->multi) {
        // swaps on level 0: (nu-1) pre + nu post, or (nuCoarse-1) when there is a single level
        const int swaps = (mg->levels == 1) ? (mg->nuCoarse - 1) : (2 * mg->nu - 1);
        double* start = (swaps % 2 == 0 || mg->smoother == 1) ? z : L0.xa;     // (Gauss-Seidel sweeps work in place: no swaps)
        double* other = (start == z) ? L0.xa : z;
        if (!mg_vcycle(mg, 0, r, start, other, done, &res)) return false;
        if (res != z) launch_copy(mg->stream, z, res, L0.n);       // not reached for the buffer choice above
        return true;
    }
    mg->finalOut = z; mg->finalWritten = false;
    const bool ok = mg_vcycle(mg, 0, r, L0.xa, L0.xb, done, &res);
    mg->finalOut = nullptr;
    if (!ok) return false;
    if (!mg->finalWritten) launch_copy(mg->stream, z, res + L0.offset, L0.n);   // (a cycle whose last step is not a Jacobi sweep: one level, one sweep)
    return true;
}

// ---------------------------------------------------------------- the CG loop
struct CgRun {
    Workspace* ws = nullptr;
    SpmvConfig cfg;
    MgcgComm* comm = nullptr;
    HaloPlan* halo = nullptr;
    MgcgMg* mg = nullptr;
    const double* dinv = nullptr;          // Jacobi-preconditioned loop (SolveJacobi*): D^-1 of the local rows; z = dinv * r is formed inside the vector passes
    const double* elements = nullptr; const int* rowOffsets = nullptr; const int* columnIndeces = nullptr;
    int elementsCount = 0;
    double *x = nullptr, *b = nullptr, *Ap = nullptr, *p = nullptr, *r = nullptr, *z = nullptr;  // p is FULL length (count), the rest local
    long long count = 0, nLocal = 0, offset = 0;
    int nranks = 1;
    bool multi = false;                    // comm_multi(comm)
    double tol = 0; int minIt = 0, maxIt = 0, rule = 0;
    bool wantInf = false;
    SpmvProfile* prof = nullptr;
    const DcsrMatrix* dcsr = nullptr;      // compressed form of the matrix if the handle has one
    MgcgSparse* cusparse = nullptr;
    double usShape = 0, usForm = 0;        // what cg_matrix_setup took (MGCG_VERBOSE=2)
    // rows [interior0, interior1) reference local columns only: they are multiplied (side stream) while the halo of p is in flight
    bool overlap = false;
    long long interior0 = 0, interior1 = 0;
    bool haloOnSide = false;               // tuning knob, resolved once per solve (every iteration of every rank takes the same path)
    Vector* pVec = nullptr;                // the handles behind p and Ap (the placement draw may move their data)
    Vector* ApVec = nullptr;
    // deferred x update (MGCG_X_DEFER, cg_xdefer_setup): groups of xDefer iterations, the host's position in the current group
    int xDefer = 1;
    int groupPos = 0, groupLen = 1;
    RingArgs ring{};
};

static thread_local long long t_lastOverlap[3] = { 0, 0, 0 };

static bool cg_plan_overlap(CgRun& R)
{
    t_lastOverlap[0] = 0; t_lastOverlap[1] = 0; t_lastOverlap[2] = 0;
    if (!plan_overlap(R.ws->stream, R.comm, R.multi, R.rowOffsets, R.columnIndeces, R.nLocal, R.offset, &R.overlap, &R.interior0, &R.interior1, R.ws->devInts + 6, R.halo, R.p, R.count)) return false;
    if (R.overlap) { t_lastOverlap[0] = 1; t_lastOverlap[1] = R.interior0; t_lastOverlap[2] = R.interior1; }
    return true;
}

static void prof_mark(CgRun& R, bool begin)
{
    SpmvProfile* p = R.prof;
    if (!p || !p->enabled) return;
    if (begin) {
        if (p->used >= (int)p->start.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            p->start.push_back(a); p->stop.push_back(b);
        }
        (void)hipEventRecord(p->start[p->used], R.ws->stream);
    } else if (p->used < (int)p->start.size()) {
        (void)hipEventRecord(p->stop[p->used], R.ws->stream);
        p->used++;
    }
}

__global__ void snapshot_kernel(const CgScalars* sc, HostMirror* m, volatile int* slot)
{
    *slot = sc->done;
    m->residual = sc->residual;
}

__global__ void clear_done_kernel(CgScalars* sc) { sc->done = 0; sc->status = 0; sc->pSlot = 0; }

// ---------------------------------------------------------------- deferred x update (MGCG_X_DEFER)
// Nothing in the loop reads x: it only has to be right when the call returns.  With B > 1 the one-rank plain loop keeps the directions of
// a group of B iterations in a ring of B buffers (slot 0 the caller's p, slots 1 .. B-1 on the workspace) and the group's last iteration
// applies x += alpha_j p_j for the whole group, oldest first -- the same rounded products and sums as one term per iteration, so x is the
// same bit for bit, and r, p, Ap and every dot are untouched.  The update pass then moves 24N bytes on B-1 iterations of B and
// (B + 4) 8N on the last one: 32N + 8N/B per iteration against 40N.
// Groups: CgSteps(K) puts the short group (K mod B) first, so that its last iteration is a flush and writes p into the caller's buffer;
// Solve groups from its first iteration, and the iteration that stops the loop flushes; if p then sits in a library slot it is copied back
// once at the end of the call (ring_copy_back_kernel).  Several ranks and the preconditioned loops keep one term per iteration.
static int cg_xdefer_slots(const CgRun& R)
{
    int B = tuning().xDefer.load(std::memory_order_relaxed);
    B = B < 1 ? 1 : (B > kXDeferMax ? kXDeferMax : B);
    const bool eligible = !R.multi && !R.mg && !R.dinv && R.nLocal > 0 && R.offset == 0 && R.count == R.nLocal;
    return eligible ? B : 1;
}

// steps: the call's iteration count when it is known (CgSteps), else 0
static void cg_xdefer_setup(CgRun& R, long long steps)
{
    R.xDefer = 1; R.groupPos = 0; R.groupLen = 1;
    const int B = cg_xdefer_slots(R);
    if (B <= 1) return;
    const bool report = tuning().verbose.load(std::memory_order_relaxed) >= 2;
    if (!R.ws->ensure_ring(B, R.nLocal)) {         // no room for the ring: one term per iteration, as with B = 1
        if (report) fprintf(stderr, "[MgcgGpu] solve set-up: deferred x update off (the ring of %d more vectors of %lld entries could not be allocated)\n", B - 1, R.nLocal);
        return;
    }
    R.ring = RingArgs{};
    R.ring.slot[0] = R.p;
    for (int i = 1; i < B; ++i) R.ring.slot[i] = R.ws->ring[i];
    R.xDefer = B;
    R.groupLen = (steps > 0 && steps % B != 0) ? (int)(steps % B) : B;
    if (report) fprintf(stderr, "[MgcgGpu] solve set-up: deferred x update in groups of %d (first group %d)\n", B, R.groupLen);
}

// ---------------------------------------------------------------- placement draw for Ap and p
// The same SpMV binary on the same matrix runs up to 17 % apart depending on WHERE the runtime placed its two vectors (identical HBM
// traffic and L2 hit rates: the timing of the same requests -- the channel / bank hash of the physical pages).  Round 4's probe
// (tools/placement_probe2.py, profiles/r4/placement_probe2.log: every pair of 4 x and 4 y allocations in one process) shows the WRITTEN
// vector dominating -- one y allocation is good or bad with every x (2.23-2.28 against 2.48-2.62 ms) -- and the gathered one adding a
// few per cent.  A kernel cannot steer that, but the library owns every vector (Create_Double): at the first solve on vectors of at
// least kPlacementMinEntries entries (256 MB: beyond the Infinity Cache) it allocates `placement` more buffers for Ap, times the loop's
// own SpMV (fused with p.Ap) on each and keeps the fastest, then does the same for p: one draw becomes the best of k, twice.
// One-off cost at 512^3: 2 x 4 candidates x 7 launches x 2.4 ms + 3 GiB of copies ~ 0.14 s, inside the first solve (the role cuSPARSE's
// csrmv analysis plays in the reference's stack).  Nothing numerical changes: the same doubles at another address.  A vector whose
// address the caller has seen (ToRawPtr_Double) is never moved.
constexpr long long kPlacementMinEntries = 32LL << 20;
static thread_local double t_placementMs[2][16];
static thread_local int t_placementInfo[2][2] = { { 0, -1 }, { 0, -1 } };     // per stage (0: Ap, 1: p): candidates timed, chosen

static void placement_report(int stage, const Vector* v)
{
    t_placementInfo[stage][0] = v ? v->drawCount : 0; t_placementInfo[stage][1] = v ? v->drawChosen : -1;
    for (int i = 0; v && i < v->drawCount && i < 16; ++i) t_placementMs[stage][i] = v->drawMs[i];
}

// The loop's SpMV (fused with p.Ap) on this run's matrix: x gathered, y written.
static SpmvArgs cg_spmv_args(const CgRun& R, const double* x, double* y)
{
    SpmvArgs a{};
    a.elements = R.elements; a.rowOffsets = R.rowOffsets; a.columnIndeces = R.columnIndeces; a.x = x; a.y = y;
    a.elementsCount = R.elementsCount; a.rowCount = (int)R.nLocal; a.columnCount = (int)R.count;
    return a;
}

// The two halves of a draw.  Candidates: up to `want` more buffers of `bytes` bytes appended to cand[n...], as long as 2 GiB stay free.
static int placement_alloc(double** cand, int n, int want, size_t bytes)
{
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (int i = 0; i < want && freeB > (size_t)(i + 1) * bytes + (2ULL << 30); ++i) {
        double* q = nullptr;
        if (hipMalloc((void**)&q, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        cand[n++] = q;
    }
    return n;
}
// Timing: the contents of src copied into cand[from..n), then the loop's SpMV on every candidate as the gathered vector (asX) or the written
// one -- one warm-up and kReps timed launches each; ms[i] per launch.  false: some call failed and ms means nothing.
static bool placement_time(CgRun& R, double* const* cand, int from, int n, const double* src, size_t bytes, bool asX, double* ms)
{
    hipStream_t s = R.ws->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = n > from && MGCG_HIP(hipEventCreate(&e0)) && MGCG_HIP(hipEventCreate(&e1));
    for (int i = from; ok && i < n; ++i) ok = MGCG_HIP(hipMemcpyAsync(cand[i], src, bytes, hipMemcpyDeviceToDevice, s));   // the same contents everywhere
    constexpr int kReps = 6;
    for (int i = 0; ok && i < n; ++i) {
        SpmvArgs a = cg_spmv_args(R, asX ? cand[i] : R.p, asX ? R.Ap : cand[i]);
        a.w = a.x + R.offset; a.partials = R.ws->partials; a.doneFlag = nullptr;
        (void)launch_spmv_auto(s, EPI_DOT, a, R.cfg, R.dcsr);                              // warm-up (Ap and the partial sums are rewritten by the solve)
        ok = MGCG_HIP(hipEventRecord(e0, s));
        for (int k = 0; k < kReps; ++k) (void)launch_spmv_auto(s, EPI_DOT, a, R.cfg, R.dcsr);
        ok = ok && MGCG_HIP(hipEventRecord(e1, s)) && MGCG_HIP(hipEventSynchronize(e1));
        float t = 0.0f;
        ok = ok && MGCG_HIP(hipEventElapsedTime(&t, e0, e1));
        ms[i] = (double)t / kReps;
    }
    (void)hipStreamSynchronize(s);
    if (!ok) (void)hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ok;
}

// one stage: candidates for vector v (stage 0: the SpMV's output Ap, whose contents do not matter at this point; stage 1: its input p);
// the fastest stays, in place of v's own buffer if it is another
static void placement_stage(CgRun& R, int stage, Vector* v)
{
    placement_report(stage, v);                    // MgcgLastPlacement speaks of THIS solve's vectors: the record of their one draw, or nothing
    const int extra = tuning().placement.load(std::memory_order_relaxed);
    double*& mine = stage == 0 ? R.Ap : R.p;
    if (!v || v->placed || v->rawExported || extra <= 0 || v->size < kPlacementMinEntries || v->data != mine || R.nLocal < 4096 || R.elementsCount < 8) return;
    v->placed = true;                              // one draw per vector, whatever comes of it
    const size_t bytes = sizeof(double) * (size_t)v->size;
    double* cand[16];
    cand[0] = v->data;
    const int n = placement_alloc(cand, 1, extra > 15 ? 15 : extra, bytes);
    if (n < 0) return;
    double ms[16];
    const bool ok = placement_time(R, cand, 1, n, v->data, bytes, stage == 1, ms);
    int best = 0;
    for (int i = 1; ok && i < n; ++i) if (ms[i] < ms[best]) best = i;
    for (int i = 0; i < n; ++i) if (i != best) { analysis_note_write(cand[i], bytes); if (i == 0) vector_registry_remove(cand[0]); (void)hipFree(cand[i]); }   // (freed addresses may be handed out again)
    if (best != 0) { v->data = cand[best]; mine = v->data; vector_registry_add(v->data, bytes); }
    if (ok) { v->drawCount = n; v->drawChosen = best; for (int i = 0; i < n; ++i) v->drawMs[i] = (float)ms[i]; placement_report(stage, v); }
    if (ok && tuning().verbose.load(std::memory_order_relaxed) >= 1) {
        fprintf(stderr, "[MgcgGpu] placement draw for %s (%lld entries): SpMV", stage == 0 ? "Ap" : "p", v->size);
        for (int i = 0; i < n; ++i) fprintf(stderr, " %.3f", ms[i]);
        fprintf(stderr, " ms -> candidate %d\n", best);
    }
}

// Is the draw worth its price for THIS call?  It costs about 2 stages x 3 candidates x 7 launches = 42 SpMV times (+ 3 GiB of copies at 512^3:
// 0.14 s in all) and wins about 4-5 % of one SpMV per iteration (profiles/r4/placement_ab_*.log): it pays from about a thousand iterations.
// The preconditioned loop converges in a few hundred (config 3: 157, where the draw recovered 28 ms of its 140: ADVICE r4) -- no draw there;
// the plain loop draws when its iteration cap leaves room for that many (the 512^3 system needs 1225), and CgSteps -- the fixed-length
// form a caller uses to time the steady state -- always does (steps = 0 in R.maxIt).
constexpr int kPlacementMinIterations = 1000;

// The deferred x update's ring (cg_xdefer_setup): the SpMV gathers from its B - 1 library-owned slots in turn, and each of them moves it as
// much as p's own placement does (in the loop at 512^3: 2.43 ms on the best of p's 4 candidates, 2.45-2.47 and 2.52 ms on ring slots drawn
// as the best 7 of 10 -- profiles/r6).  So they are drawn the way p is, best of (1 + `placement`) per slot: (B - 1)(1 + placement)
// allocations (at most 16) timed as the gathered vector, the B - 1 fastest kept in ascending time -- once per workspace, when the ring is
// first needed at this size.  MgcgLastPlacement keeps reporting the two stages above; MGCG_VERBOSE=1 prints this one.
static void placement_ring(CgRun& R)
{
    const int B = cg_xdefer_slots(R);
    const int extra = tuning().placement.load(std::memory_order_relaxed);
    Workspace* ws = R.ws;
    if (B <= 1 || extra <= 0 || R.nLocal < kPlacementMinEntries || R.elementsCount < 8) return;
    if (ws->ringSize >= R.nLocal) { bool some = false; for (int i = 1; i < kXDeferMax; ++i) some = some || ws->ring[i] != nullptr; if (some) return; }
    (void)hipStreamSynchronize(ws->stream);
    ws->free_ring();
    const size_t bytes = sizeof(double) * (size_t)R.nLocal;
    double* cand[16];
    const int n = placement_alloc(cand, 0, (B - 1) * (1 + extra) > 16 ? 16 : (B - 1) * (1 + extra), bytes);
    if (n < 0) return;
    double ms[16];
    int order[16];
    const bool ok = placement_time(R, cand, 0, n, R.p, bytes, true, ms);
    for (int i = 0; i < n; ++i) { order[i] = i; if (!ok) ms[i] = (double)i; }
    std::stable_sort(order, order + n, [&](int a, int b) { return ms[a] < ms[b]; });
    const int take = n < B - 1 ? n : B - 1;
    ws->ringSize = R.nLocal;
    for (int k = 0; k < take; ++k) ws->ring[1 + k] = cand[order[k]];
    for (int k = take; k < n; ++k) (void)hipFree(cand[order[k]]);
    if (ok && tuning().verbose.load(std::memory_order_relaxed) >= 1) {
        fprintf(stderr, "[MgcgGpu] placement draw for the ring of p (%d slots): SpMV", B - 1);
        for (int i = 0; i < n; ++i) fprintf(stderr, " %.3f", ms[i]);
        fprintf(stderr, " ms -> candidates");
        for (int k = 0; k < take; ++k) fprintf(stderr, " %d", order[k]);
        fprintf(stderr, "\n");
    }
}
static void placement_draw(CgRun& R, bool fixedSteps)
{
    if (R.mg != nullptr || R.dinv != nullptr || (!fixedSteps && R.maxIt < kPlacementMinIterations)) { placement_report(0, nullptr); placement_report(1, nullptr); return; }
    placement_stage(R, 0, R.ApVec);                // the written vector first: it decides the most
    placement_stage(R, 1, R.pVec);
    placement_ring(R);
}

// What the loop's SpMV needs to know about this call's matrix: its shape, its compressed form if the handle has one, and the kernel flags
// that follow.  Once per call.
static void cg_matrix_setup(CgRun& R)
{
    long long meanDistance = 0;
    auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count(); };
    const auto t0 = std::chrono::steady_clock::now();
    if (R.elementsCount >= 8) R.cfg.periodRows = spmv_period(R.cusparse, R.rowOffsets, R.columnIndeces, R.nLocal, R.offset, &R.cfg.maxRow, &meanDistance);
    R.usShape = since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    R.dcsr = dcsr_lookup(R.cusparse, R.elements, R.rowOffsets, R.columnIndeces, R.nLocal, R.elementsCount, R.offset, R.count, R.mg ? -1 : meanDistance);
    R.usForm = since(t1);
    if (meanDistance >= (1LL << 19) && R.count >= (8LL << 19)) R.cfg.flags |= 16;      // gathers without locality: the stream form among the CSR kernels
    if (!R.mg) R.cfg.flags |= 8;                 // plain CG loop: the row-tile kernel may read the matrix with the non-temporal hint (kernels_rowtile.hip)
}

static bool cg_enqueue_init(CgRun& R, bool fixedSteps = false)
{
    hipStream_t s = R.ws->stream;
    // MGCG_VERBOSE=2: what a solve pays before its first iteration is enqueued (the reference's driver times a cold Solve(): MgcgMain.cs:121-126)
    const auto t2 = std::chrono::steady_clock::now();
    placement_draw(R, fixedSteps);               // (before p is touched: may move p's data once per vector)
    if (tuning().verbose.load(std::memory_order_relaxed) >= 2)
        fprintf(stderr, "[MgcgGpu] solve set-up: matrix shape %.0f us, matrix form %.0f us, placement draw %.0f us\n", R.usShape, R.usForm,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t2).count());
    CgScalars* sc = R.ws->scalars;
    double* pLoc = R.p + R.offset;
    if (R.rule == MGCG_RULE_SIMPLE) launch_fill(s, R.x, 0.0, R.nLocal);             // SimpleConjugateGradient.cu:53
    launch_copy(s, pLoc, R.x, R.nLocal);                                             // p_loc = x  (Mgcg.cu:80)
    if (!halo_exchange(R.comm, R.halo, R.p, s)) return false;                        // SyncP  (ConjugateGradientParallelGpu.cs:427)
    SpmvArgs a = cg_spmv_args(R, R.p, R.r);
    a.b = R.b;
    launch_spmv_auto(s, EPI_RESIDUAL, a, R.cfg, R.dcsr);                             // r = b - A x   (Mgcg.cu:225-226)
    // The partial sums of what alpha and beta divide: r.r, or r.z with the V-cycle.  The Jacobi loop keeps r.z next to the true r.r, which
    // its relative stop rule divides by (the start pass runs at most kMaxGrid <= kMaxPartials / 2 workgroups).
    double* partials = R.ws->partials;
    double* partialsZ = R.dinv ? partials + kMaxPartials / 2 : nullptr;
    int n;
    if (R.mg) {
        int nz = 0;
        if (!mg_apply(R.mg, R.r, R.z, nullptr, dot_reference_order() ? nullptr : partials, &nz)) return false;   // z = M^-1 r (+ r.z)
        launch_copy(s, pLoc, R.z, R.nLocal);                                         // p = z
        n = nz > 0 ? nz : launch_dot_partials(s, R.r, R.z, R.nLocal, partials);      // rz = r.z
    } else {
        n = launch_copy_dot(s, pLoc, R.r, R.dinv, R.nLocal, partials, partialsZ, nullptr);   // p = r ; rr = r.r  (Mgcg.cu:227-228), or p = z = D^-1 r ; r.r and r.z
    }
    if (R.multi) {                                                                   // resultsDot.Sum()  (:463); the Jacobi loop's pair {rrNew, rzNew} in one all-reduce
        if (R.dinv) launch_reduce2_to(s, partials, n, &sc->rrNew, partialsZ, n, &sc->rzNew, nullptr);
        else launch_reduce_to(s, partials, n, &sc->rr, nullptr);
        if (!comm_allreduce_sum(R.comm, R.dinv ? &sc->rrNew : &sc->rr, R.dinv ? 2 : 1, s)) return false;
    }
    launch_init_scalars(s, partials, partialsZ, n, !R.multi, sc, R.ws->mirror);
    return MGCG_HIP(hipGetLastError());
}

// The product step of one iteration: SyncP, Ap = A p with the partial sums of p.Ap in ws->partials[0 .. *nPAp).  pIn: the vector that
// holds p_k (the caller's p, or a slot of the deferred x update's ring).  w: the local rows of the vector the sum is taken with, w.Ap (null: p
// itself, p.Ap; the BiCGStab loop sums rhat.v and s.t).
static bool cg_enqueue_product(CgRun& R, double* pIn, int* nPAp, const double* w = nullptr)
{
    hipStream_t s = R.ws->stream;
    const int* done = &R.ws->scalars->done;
    SpmvArgs a = cg_spmv_args(R, pIn, R.Ap);
    a.w = w ? w : pIn + R.offset; a.partials = R.ws->partials; a.doneFlag = done;
    int n;
    if (R.overlap) {
        // interior rows on the side stream while SyncP (:469) travels on the main stream, then the boundary rows
        prof_mark(R, true);
        hipStream_t side = halo_overlap_fork(R.comm, s);
        if (!side) return false;
        if (R.haloOnSide) {
            // SyncP (:469) on the side stream, all rows on the main stream: the two cross-stream hops (10 us each, measured) and the wire
            // time of the planes hide behind the interior rows; the join finds the exchange long finished
            if (!halo_exchange(R.comm, R.halo, R.p, side)) return false;
            n = launch_spmv_range(s, EPI_DOT, a, R.cfg, R.dcsr, R.interior0, R.interior1, R.ws->partials, kMaxPartials / 2);
            if (!halo_overlap_join(R.comm, s)) return false;
            n += launch_spmv_two_ranges(s, EPI_DOT, a, R.cfg, R.dcsr, R.interior0, R.interior1, R.ws->partials + n, kMaxPartials / 2);   // boundary rows: one launch when the cuts fall on tiles
        } else {
            n = launch_spmv_range(side, EPI_DOT, a, R.cfg, R.dcsr, R.interior0, R.interior1, R.ws->partials, kMaxPartials / 2);
            if (!halo_exchange(R.comm, R.halo, R.p, s)) return false;
            n += launch_spmv_two_ranges(s, EPI_DOT, a, R.cfg, R.dcsr, R.interior0, R.interior1, R.ws->partials + n, kMaxPartials / 2);
            if (!halo_overlap_join(R.comm, s)) return false;
        }
        prof_mark(R, false);
    } else {
        if (!halo_exchange(R.comm, R.halo, R.p, s)) return false;                    // SyncP  (:469)
        prof_mark(R, true);
        n = launch_spmv_auto(s, EPI_DOT, a, R.cfg, R.dcsr);                          // Ap = A p ; p.Ap   (Mgcg.cu:244-245)
        prof_mark(R, false);
    }
    if (dot_reference_order()) { launch_dot_serial(s, a.w, R.Ap, R.nLocal, R.ws->partials, done); n = 1; }   // validation mode: p.Ap once more, in the reference's order
    *nPAp = n;
    return true;
}

// What follows the product in one iteration.  Every variant starts with update_r (alpha, r -= alpha Ap, partial r.r); they differ in who
// takes the stop decision and where x and p are updated.  The Jacobi loop (R.dinv) takes the Fused and Unfused rows: update_r and
// update_xp_final form z = D^-1 r themselves, and r.z travels with r.r (reduce2, [r.r, r.z] in place of reduce, [r.r]).
// Launches per iteration after the product, all-reduces in brackets:
enum class CgUpdate {
    FusedOneRank,       // update_r, update_xp_final (or update_xp_ring: deferred x update)                                          2
    FusedRanks,         // reduce, [p.Ap], update_r, reduce, [r.r], update_xp_final                                                 4
    PrecondOneRank,     // update_r, finalize, V-cycle (+ dot), finalize_precond, update_xp                                         4 + V-cycle
    PrecondRanks,       // reduce, [p.Ap], update_r, V-cycle (+ dot), reduce2, [r.r, r.z], finalize, update_xp                      5 + V-cycle
    Unfused             // a rank without rows: as the Fused variants, with finalize in place of the x/p update (Jacobi: reduce2 in front)   2 to 4
};
static CgUpdate cg_update_variant(const CgRun& R)
{
    if (R.mg) return R.multi ? CgUpdate::PrecondRanks : CgUpdate::PrecondOneRank;
    // a rank without rows: launch_update_xp_final returns before it launches (n <= 0), so only launch_finalize can finalise its iteration
    if (R.nLocal <= 0) return CgUpdate::Unfused;
    return R.multi ? CgUpdate::FusedRanks : CgUpdate::FusedOneRank;
}

static FinalizeArgs cg_finalize_args(const CgRun& R, bool withStopTest, int preconditioned)
{
    FinalizeArgs f{};
    f.sc = R.ws->scalars; f.mirror = R.ws->mirror; f.trace = R.ws->trace; f.traceCap = R.ws->traceCap;
    f.tol = R.tol; f.minIt = R.minIt; f.maxIt = R.maxIt; f.rule = R.rule; f.preconditioned = preconditioned;
    if (!withStopTest) { f.tol = -1.0; f.minIt = 0; f.maxIt = 0x7fffffff; f.rule = MGCG_RULE_NATIVE; }   // never converges
    return f;
}

// The update step.  pLoc: this rank's rows of p_k; nPAp: the product step's count of p.Ap partial sums.
static bool cg_enqueue_update(CgRun& R, double* pLoc, int nPAp, bool withStopTest)
{
    hipStream_t s = R.ws->stream;
    CgScalars* sc = R.ws->scalars;
    const int* done = &sc->done;
    const CgUpdate variant = cg_update_variant(R);
    const bool fused = variant == CgUpdate::FusedOneRank || variant == CgUpdate::FusedRanks;   // update_r freezes the scalars for update_xp_final / _ring
    const bool refDots = dot_reference_order();
    double* pInf = R.wantInf ? R.ws->partials + kMaxPartials : nullptr;
    // the r update leaves its partial sums of r.r and, in the Jacobi loop, of r.z in the third region of the buffer (its grid is a few hundred
    // workgroups; with the V-cycle they must outlive it: its r.z partial sums take the first region)
    double* rrPartials = R.ws->partials + 2 * kMaxPartials;
    double* rzPartials = R.dinv ? rrPartials + kMaxPartials / 2 : nullptr;
    if (R.multi) {
        launch_reduce_to(s, R.ws->partials, nPAp, &sc->pAp, done);
        if (!comm_allreduce_sum(R.comm, &sc->pAp, 1, s)) return false;               // (:499)
    }
    // r -= a Ap ; r.r  (:247-248); x += a p rides with the p update below.  One rank: the workgroups of the r update add the p.Ap partial sums
    // themselves (one launch fewer per iteration)
    int n = launch_update_r(s, sc, R.r, R.Ap, R.dinv, R.nLocal, rrPartials, rzPartials, pInf, R.multi ? nullptr : R.ws->partials, R.multi ? 0 : nPAp, fused);
    if (R.dinv && (R.multi || variant == CgUpdate::Unfused)) {                       // Jacobi loop: r.r and r.z in one launch, one all-reduce of the adjacent pair
        launch_reduce2_to(s, rrPartials, n, &sc->rrNew, rzPartials, n, &sc->rzNew, done);
        if (R.multi && !comm_allreduce_sum(R.comm, &sc->rrNew, 2, s)) return false;
    } else if (R.multi && !R.mg) {                                                   // plain loop of several ranks: r.r all-reduced into sc->rrNew
        launch_reduce_to(s, rrPartials, n, &sc->rrNew, done);
        if (!comm_allreduce_sum(R.comm, &sc->rrNew, 1, s)) return false;             // (:525)
    }
    const FinalizeArgs f = cg_finalize_args(R, withStopTest, (variant == CgUpdate::PrecondRanks || R.dinv) ? 2 : (R.mg ? 1 : 0));
    switch (variant) {
    case CgUpdate::FusedOneRank:
        // the x/p update finalises the iteration itself: residual, stop test, beta (:251-266) ; x += a p (:246) ; p = r + beta p (:265)
        // (Jacobi: beta = rzNew / rz ; p = D^-1 r + beta p)
        if (R.xDefer > 1) {
            RingArgs g = R.ring;
            g.pos = R.groupPos; g.flush = R.groupPos + 1 == R.groupLen ? 1 : 0;
            launch_update_xp_ring(s, f, rrPartials, pInf, n, R.x, g, R.r, R.nLocal);     // the same, x += a p once per group (cg_xdefer_setup)
            if (g.flush) { R.groupPos = 0; R.groupLen = R.xDefer; } else ++R.groupPos;
        } else {
            launch_update_xp_final(s, f, rrPartials, rzPartials, pInf, n, R.x, pLoc, R.r, R.dinv, R.nLocal);
        }
        break;
    case CgUpdate::FusedRanks:
        launch_update_xp_final(s, f, nullptr, nullptr, nullptr, 0, R.x, pLoc, R.r, R.dinv, R.nLocal);   // the same fold behind the all-reduce of r.r (Jacobi: of {r.r, r.z})
        break;
    case CgUpdate::Unfused:
        // residual, stop test, beta  (:251-266); one rank of the plain loop: it adds r.r up first (Jacobi, preconditioned = 2: {rrNew, rzNew} are in place)
        launch_finalize(s, rrPartials, pInf, n, !R.multi && !R.dinv, f);
        launch_update_xp(s, sc, R.x, pLoc, R.r, R.nLocal);                           // x += a p (:246) ; p = r + beta p   (:265) -- returns at once without rows
        break;
    case CgUpdate::PrecondOneRank: {
        launch_finalize(s, rrPartials, pInf, n, true, f);                            // residual, stop test  (:251-266)
        int nz = 0;
        if (!mg_apply(R.mg, R.r, R.z, done, refDots ? nullptr : R.ws->partials, &nz)) return false;   // z = M^-1 r (+ r.z on the last sweep)
        n = nz > 0 ? nz : launch_dot_partials(s, R.r, R.z, R.nLocal, R.ws->partials);
        launch_finalize_precond(s, R.ws->partials, n, true, sc);                     // beta = rzNew / rz
        launch_update_xp(s, sc, R.x, pLoc, R.z, R.nLocal);                           // x += a p (:246) ; p = z + beta p
        break;
    }
    case CgUpdate::PrecondRanks: {
        // r.r (stop test) and r.z (beta) travel in ONE all-reduce of two doubles behind the V-cycle ("[r.z, r.r]
        // batched"); the stop decision of an iteration is taken one V-cycle later, which costs one wasted V-cycle at the very end and
        // saves a collective per iteration.
        const int nrr = n;
        int nz = 0;
        if (!mg_apply(R.mg, R.r, R.z, done, refDots ? nullptr : R.ws->partials, &nz)) return false;      // z = M^-1 r (+ partial sums of r.z on the last sweep)
        n = nz > 0 ? nz : launch_dot_partials(s, R.r, R.z, R.nLocal, R.ws->partials);
        launch_reduce2_to(s, rrPartials, nrr, &sc->rrNew, R.ws->partials, n, &sc->rzNew, done);   // local r.r and r.z, one launch
        if (!comm_allreduce_sum(R.comm, &sc->rrNew, 2, s)) return false;             // {rrNew, rzNew} are adjacent in CgScalars  (:525 and the PCG's r.z)
        launch_finalize(s, rrPartials, pInf, n, false, f);                           // (preconditioned = 2: also beta = rzNew / rz, rz = rzNew)
        launch_update_xp(s, sc, R.x, pLoc, R.z, R.nLocal);                           // x += a p (:246) ; p = z + beta p
        break;
    }
    }
    return MGCG_HIP(hipGetLastError());
}

static bool cg_enqueue_iteration(CgRun& R, bool withStopTest)
{
    double* pIn = R.xDefer > 1 ? R.ring.slot[R.groupPos] : R.p;                      // the slot that holds p_k (deferred x update)
    int nPAp = 0;
    return cg_enqueue_product(R, pIn, &nPAp) && cg_enqueue_update(R, pIn + R.offset, nPAp, withStopTest);
}

// The host's side of a device-resident loop.  It enqueues checkEvery iterations, a snapshot of the device's stop flag and an event, and then
// looks at the snapshot of the chunk BEFORE the one just enqueued, so that the device never waits for the host.  A loop whose flag has not
// risen a little beyond max(minIt, maxIt) iterations is an error (who names the loop in the message).  The stream is not drained here.
// snapshot(slot) enqueues the launch that copies the loop's device stop flag into the pinned int *slot.
template <typename Enqueue, typename Snapshot>
static bool cg_drive_on(CgRun& R, const char* who, Enqueue enqueueIteration, Snapshot snapshot, long long* enqueuedOut = nullptr)
{
    hipStream_t s = R.ws->stream;
    int checkEvery = 4;
    { const int v = tuning().checkEvery.load(std::memory_order_relaxed); if (v >= 1) checkEvery = v; }
    const long long hostCap = (long long)(R.maxIt > R.minIt ? R.maxIt : R.minIt) + 4;
    hipEvent_t ev[2] = { nullptr, nullptr };
    volatile int* slots = (volatile int*)&R.ws->hostScalar[2];   // two ints per double: slots[0..3]
    bool ok = MGCG_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming)) && MGCG_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    for (int i = 0; i < 4; ++i) slots[i] = 0;
    long long enqueued = 0;
    int chunk = 0;
    bool finished = false;
    while (ok && !finished) {
        for (int k = 0; ok && k < checkEvery; ++k) ok = enqueueIteration();
        enqueued += checkEvery;
        snapshot(&slots[chunk & 1]);
        ok = ok && MGCG_HIP(hipEventRecord(ev[chunk & 1], s));
        if (chunk > 0) {                                  // look at the chunk BEFORE the one just enqueued
            ok = ok && MGCG_HIP(hipEventSynchronize(ev[(chunk - 1) & 1]));
            if (ok && slots[(chunk - 1) & 1] != 0) finished = true;
        }
        if (!finished && enqueued > hostCap + 2LL * checkEvery) {
            ok = ok && MGCG_HIP(hipStreamSynchronize(s));
            if (ok && slots[chunk & 1] != 0) finished = true;
            else { set_error("%s: the device never raised its stop flag after %lld iterations", who, enqueued); ok = false; }
        }
        ++chunk;
    }
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (enqueuedOut) *enqueuedOut = enqueued;
    return ok;
}
// The loops whose stop flag is CgScalars::done: their snapshot also mirrors the residual.
template <typename Enqueue>
static bool cg_drive(CgRun& R, const char* who, Enqueue enqueueIteration, long long* enqueuedOut = nullptr)
{
    return cg_drive_on(R, who, enqueueIteration, [&](volatile int* slot) {
        hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(1), 0, R.ws->stream, R.ws->scalars, R.ws->mirror, slot);
    }, enqueuedOut);
}

// cg_drive for the variants' loops: body(k) enqueues body k and returns false when it could not; k is the host's count, which saturates at INT_MAX,
// and the launches' errors are looked at behind every body.
template <typename Body>
static bool cg_drive_bodies(CgRun& R, const char* who, Body body)
{
    int k = 0;
    return cg_drive(R, who, [&] {
        if (!body(k)) return false;
        if (k < 0x7fffffff) ++k;
        return MGCG_HIP(hipGetLastError());
    });
}

static int cg_solve(CgRun& R, int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    hipStream_t s = R.ws->stream;
    HostMirror* m = R.ws->mirror;
    if (R.rule < MGCG_RULE_NATIVE || R.rule > MGCG_RULE_VIENNACL) { set_error("unknown stop rule %d", R.rule); return MGCG_ERROR; }
    R.wantInf = (R.rule == MGCG_RULE_HANDMADECL);
    if (R.wantInf && R.nranks > 1) { set_error("the max-norm rule is single-rank only"); return MGCG_ERROR; }
    if (residualTrace && traceCapacity > 0) { if (!R.ws->ensure_trace(traceCapacity)) return MGCG_ERROR; }
    const int devTraceCap = (residualTrace && traceCapacity > 0) ? traceCapacity : 0;
    double* savedTrace = R.ws->trace; const int savedCap = R.ws->traceCap;
    if (!devTraceCap) { R.ws->trace = nullptr; R.ws->traceCap = 0; } else R.ws->traceCap = devTraceCap;

    R.haloOnSide = tuning().haloStream.load(std::memory_order_relaxed) != 0;
    int status = MGCG_ERROR;
    const bool report = tuning().verbose.load(std::memory_order_relaxed) >= 2;
    const auto hostT0 = std::chrono::steady_clock::now();
    cg_matrix_setup(R);
    bool ok = cg_enqueue_init(R);
    if (ok) cg_xdefer_setup(R, 0);
    if (report) {
        const double enq = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT0).count();
        (void)hipStreamSynchronize(s);
        fprintf(stderr, "[MgcgGpu] solve: initial phase enqueued after %.0f us, finished on the device after %.0f us\n", enq,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT0).count());
    }
    long long enqueued = 0;
    ok = ok && cg_drive(R, "CG", [&] { return cg_enqueue_iteration(R, true); }, &enqueued);
    if (ok && R.xDefer > 1) launch_ring_copy_back(s, R.ws->scalars, R.ring, R.nLocal);   // p stopped inside a group: back into the caller's buffer
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (report) fprintf(stderr, "[MgcgGpu] solve: %lld iterations enqueued, loop drained %.0f us after the call began\n", enqueued,
                        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT0).count());
    if (ok) {
        status = m->status;
        if (iteration) *iteration = m->iteration;
        if (residual) *residual = m->residual;
        if (devTraceCap) {
            int nTrace = m->iteration + 1; if (nTrace > devTraceCap) nTrace = devTraceCap;
            ok = MGCG_HIP(hipMemcpy(residualTrace, R.ws->trace, sizeof(double) * (size_t)nTrace, hipMemcpyDeviceToHost));
        }
        if (status == MGCG_MAXIT_EXCEEDED) set_error("CG did not converge: iteration %d exceeded maxIteration %d (residual %g)", m->iteration, R.maxIt, m->residual);
        if (status == MGCG_NONFINITE) set_error("CG stopped: residual is not finite at iteration %d", m->iteration);
    }
    R.ws->trace = savedTrace; R.ws->traceCap = savedCap;
    return ok ? status : MGCG_ERROR;
}

// ---------------------------------------------------------------- what the variant loops share
// The device trace of a loop of k columns, each of the caller's capacity: room on the workspace, and f told where it is.  f.traceCap is 0 afterwards
// when the caller wants no trace.
static bool cg_trace_columns(Workspace* ws, int k, const double* residualTrace, int traceCapacity, FinalizeArgs& f)
{
    f.traceCap = (residualTrace && traceCapacity > 0) ? traceCapacity : 0;
    if (f.traceCap && !ws->ensure_trace(k * f.traceCap)) return false;
    f.trace = f.traceCap ? ws->trace : nullptr;
    return true;
}

// What a loop of k columns hands back: column j's iteration (hIteration null: the loop has one count for all), residual and status into the
// caller's arrays (each may be null), and the first nTrace[j] (null: hIteration[j] + 1) entries of its device trace to residualTrace + j * traceCapacity.
// Returns the worst status, NONFINITE over MAXIT_EXCEEDED over OK; *ok falls when a copy fails.
static int cg_return_columns(Workspace* ws, int k, const int hIteration[], const double hResidual[], const int hStatus[], const int nTrace[], int devTraceCap,
                             int iteration[], double residual[], int status[], double* residualTrace, int traceCapacity, bool* ok)
{
    int worst = MGCG_OK;
    for (int j = 0; *ok && j < k; ++j) {
        if (iteration && hIteration) iteration[j] = hIteration[j];
        if (residual) residual[j] = hResidual[j];
        if (status) status[j] = hStatus[j];
        if (hStatus[j] == MGCG_NONFINITE) worst = MGCG_NONFINITE;
        else if (hStatus[j] == MGCG_MAXIT_EXCEEDED && worst == MGCG_OK) worst = MGCG_MAXIT_EXCEEDED;
        int n = nTrace ? nTrace[j] : hIteration[j] + 1; if (n > devTraceCap) n = devTraceCap;
        if (n > 0) *ok = MGCG_HIP(hipMemcpy(residualTrace + (size_t)j * traceCapacity, ws->trace + (size_t)j * devTraceCap, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return worst;
}
// ... and the message that goes with the worst status (nonfinite: what MGCG_NONFINITE means in this loop)
static void cg_columns_message(const char* who, int worst, const char* nonfinite, int maxIt)
{
    if (worst == MGCG_NONFINITE) set_error("%s: %s", who, nonfinite);
    else if (worst == MGCG_MAXIT_EXCEEDED) set_error("%s: a column did not converge within maxIteration %d", who, maxIt);
}

// What a one-column loop hands back once its stream has drained: iteration and residual from the mirror, the first min(iteration + 1,
// devTraceCap) entries of the device trace, and the message of a status that is not MGCG_OK.  residualName and inNorm word the residual of
// the MAXIT message ("residual" / "true residual", "" / " in the M^-1 norm"); nonfinite says what MGCG_NONFINITE means in this loop.
// Returns the status, MGCG_ERROR when the trace's copy fails.
static int cg_return_one(const CgRun& R, const char* who, int devTraceCap, int* iteration, double* residual, double* residualTrace,
                         const char* residualName, const char* inNorm, const char* nonfinite)
{
    const HostMirror* m = R.ws->mirror;
    const int it = m->iteration, status = m->status;
    const double res = m->residual;
    bool ok = true;
    cg_return_columns(R.ws, 1, &it, &res, &status, nullptr, devTraceCap, iteration, residual, nullptr, residualTrace, devTraceCap, &ok);
    if (status == MGCG_MAXIT_EXCEEDED) set_error("%s: did not converge: iteration %d exceeded maxIteration %d (%s %g%s)", who, it, R.maxIt, residualName, res, inNorm);
    if (status == MGCG_NONFINITE) set_error("%s: stopped at iteration %d: %s", who, it, nonfinite);
    return ok ? status : MGCG_ERROR;
}

// The prologue of a one-column loop that takes the plain loop's product, behind the caller's own ensure_* calls: the finalisation's
// arguments and the device trace (the last allocation: nothing is enqueued before it), the matrix set-up, every exchange kept in line (no
// overlap schedule), and x = 0 under MGCG_RULE_SIMPLE (SimpleConjugateGradient.cu:53).
static bool cg_variant_begin(CgRun& R, int preconditioned, const double* residualTrace, int traceCapacity, FinalizeArgs* f)
{
    *f = cg_finalize_args(R, true, preconditioned);
    if (!cg_trace_columns(R.ws, 1, residualTrace, traceCapacity, *f)) return false;
    cg_matrix_setup(R);
    R.overlap = false;
    if (R.rule == MGCG_RULE_SIMPLE) launch_fill(R.ws->stream, R.x, 0.0, R.nLocal);
    return true;
}

// out = b - A x through a full-length buffer: x into the rows' slice of `full`, its halo exchanged in line, the product with the residual epilogue.
// gate (the restarts of the GMRES loop): a device int, nonzero = the product writes nothing.
static bool cg_enqueue_residual(CgRun& R, double* full, double* out, const int* gate = nullptr)
{
    hipStream_t s = R.ws->stream;
    launch_copy(s, full + R.offset, R.x, R.nLocal);
    if (!halo_exchange(R.comm, R.halo, full, s)) return false;
    SpmvArgs a = cg_spmv_args(R, full, out);
    a.b = R.b; a.doneFlag = gate;
    launch_spmv_auto(s, EPI_RESIDUAL, a, R.cfg, R.dcsr);
    return true;
}

// Several ranks: this rank's partial sums -- one array, or with pB a pair whose destinations are adjacent -- folded into dst (and dst + 1)
// and all-reduced there in place.  One rank never comes here: its passes fold the partial sums themselves.
static bool cg_share_sums(CgRun& R, const double* pA, int nA, const double* pB, int nB, double* dst, const int* gate)
{
    hipStream_t s = R.ws->stream;
    if (pB) launch_reduce2_to(s, pA, nA, dst, pB, nB, dst + 1, gate);
    else launch_reduce_to(s, pA, nA, dst, gate);
    return comm_allreduce_sum(R.comm, dst, pB ? 2 : 1, s);
}

// The close of MINRES, preconditioned MINRES, BiCGStab, BiCGStab(l) and GMRES, behind the loop (ok: all of it was enqueued): t = b - A x
// through `full` into `out`; form() makes the true residual of t and leaves the partial sums of its r.r in `partials`, returning their count;
// the sum into *dst -- folded on one rank too: no pass follows that would -- all-reduced on several, and read back behind it; also(), what
// else the caller reads back; then the stream drained, *trueResidual (may be null) = the root of that sum, and cg_return_one's report.
template <typename Form>
static int cg_close_true_residual(CgRun& R, bool ok, const char* who, double* full, double* out, Form form, const double* partials, double* dst,
                                  int devTraceCap, int* iteration, double* residual, double* trueResidual, double* residualTrace,
                                  const char* inNorm, const char* nonfinite, const std::function<bool()>& also = nullptr)
{
    hipStream_t s = R.ws->stream;
    double rrTrue = 0.0;
    ok = ok && cg_enqueue_residual(R, full, out);
    if (ok) {
        const int nOut = form();
        launch_reduce_to(s, partials, nOut, dst, nullptr);
        ok = (!R.multi || comm_allreduce_sum(R.comm, dst, 1, s)) && MGCG_HIP(hipGetLastError()) &&
             MGCG_HIP(hipMemcpyAsync(&rrTrue, dst, sizeof(double), hipMemcpyDeviceToHost, s)) && (!also || also());
    }
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (!ok) return MGCG_ERROR;
    if (trueResidual) *trueResidual = std::sqrt(rrTrue);
    return cg_return_one(R, who, devTraceCap, iteration, residual, residualTrace, "residual", inNorm, nonfinite);
}

// The refusals and rules that the exports of the variants word alike.  A stop rule that is unknown or, with maxNormWhy (why this loop cannot
// take it), the max-norm rule: true, refused.
static bool cg_rule_refused(const char* who, int rule, const char* maxNormWhy)
{
    if (rule == MGCG_RULE_HANDMADECL && maxNormWhy) set_error("%s: the max-norm rule (MGCG_RULE_HANDMADECL) is not supported: %s", who, maxNormWhy);
    else if (rule < MGCG_RULE_NATIVE || rule > MGCG_RULE_VIENNACL) set_error("%s: unknown stop rule %d", who, rule);
    else return false;
    return true;
}
// The slices of a work vector (BiCGStab(l), GMRES(m)) lie this many entries apart: even, so that every slice stays 16-byte aligned
static long long cg_work_stride(long long count) { return (count + 1) & ~1LL; }
// A vector of fewer than `need` entries: true, refused.  of: what `need` counts ("local rows", "columns", "rows"), with a remark if there is one.
static bool cg_vector_short(const char* who, const char* name, const Vector* v, int need, const char* of)
{
    if (v->size >= need) return false;
    set_error("%s: the %s vector holds %lld entries, the matrix has %d %s", who, name, v->size, need, of);
    return true;
}
// R.dinv of a loop that runs with the diagonal when the caller gives one.  A rank without rows has an empty dinv vector (no data): any
// address says "with the diagonal" to the loop, which reads nothing through it there -- the ranks must agree on the form.
static double* cg_dinv_address(const CgRun& R, const Vector* dinv) { return dinv ? (dinv->data ? dinv->data : R.ws->partials) : nullptr; }
// These vectors are written by the call, n entries each (the matrix analysis must not trust a form that lies in one of them).
static void cg_note_written(std::initializer_list<double*> vectors, long long n)
{
    for (double* v : vectors) analysis_note_write(v, sizeof(double) * (size_t)n);
}

// ---------------------------------------------------------------- multi-shift CG (SolveShifted)
// One CG recurrence on A serves the k systems (A + sigma_j I) x_j = b (kernels_shift.hip has the method).  An iteration is the plain loop's
// product and r update followed by the one fused pass launch_update_shifted: three launches, as SolveEx's.  x_j starts from 0, so r = b
// exactly and no product is needed in front of the loop.  ps: the k directions p_j, column j at j * count.
static int cg_solve_shifted(CgRun& R, double* ps, int k, const double* shifts, int iteration[], double residual[], int status[],
                            double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    R.wantInf = (R.rule == MGCG_RULE_HANDMADECL);
    FinalizeArgs f = cg_finalize_args(R, true, 0);
    if (!ws->ensure_shift() || !cg_trace_columns(ws, k, residualTrace, traceCapacity, f)) return MGCG_ERROR;
    cg_matrix_setup(R);

    ShiftScalars h{};
    for (int j = 0; j < k; ++j) { h.sigma[j] = shifts[j]; h.st[0].zeta[j] = 1.0; h.st[0].zetaPrev[j] = 1.0; h.st[0].live[j] = 1; }
    h.st[0].alphaPrev = 1.0; h.st[0].betaPrev = 0.0;
    bool ok = MGCG_HIP(hipMemcpyAsync(ws->shiftScalars, &h, sizeof(h), hipMemcpyHostToDevice, s));
    launch_fill(s, R.x, 0.0, (long long)k * n);                                       // x_j = 0
    launch_copy(s, R.r, R.b, n);                                                       // r = b - A 0
    const int nRR = launch_copy_dot(s, R.p, R.r, nullptr, n, ws->partials, nullptr, nullptr);   // p = r ; r.r
    for (int j = 0; j < k; ++j) launch_copy(s, ps + j * n, R.b, n);                    // p_j = b
    launch_init_scalars(s, ws->partials, nullptr, nRR, true, ws->scalars, ws->mirror);
    ok = ok && MGCG_HIP(hipGetLastError());

    double* pInf = R.wantInf ? ws->partials + kMaxPartials : nullptr;
    double* rrPartials = ws->partials + 2 * kMaxPartials;                              // (the plain loop's regions: cg_enqueue_update)
    ok = ok && cg_drive(R, "SolveShifted", [&] {
        int nPAp = 0;
        if (!cg_enqueue_product(R, R.p, &nPAp)) return false;                          // Ap = A p ; p.Ap
        const int nP = launch_update_r(s, ws->scalars, R.r, R.Ap, nullptr, n, rrPartials, nullptr, pInf, ws->partials, nPAp, true);   // alpha ; r -= alpha Ap ; r.r
        launch_update_shifted(s, k, f, ws->shiftScalars, rrPartials, pInf, nP, R.x, R.p, R.r, ps, n);
        return MGCG_HIP(hipGetLastError());
    });
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    ok = ok && MGCG_HIP(hipMemcpy(&h, ws->shiftScalars, sizeof(h), hipMemcpyDeviceToHost));
    if (!ok) return MGCG_ERROR;
    const int worst = cg_return_columns(ws, k, h.iteration, h.residual, h.status, nullptr, f.traceCap, iteration, residual, status, residualTrace, traceCapacity, &ok);
    if (ok) cg_columns_message("SolveShifted", worst, "a column broke down (p.Ap <= 0 or a scalar that is not finite)", R.maxIt);
    return ok ? worst : MGCG_ERROR;
}

// ---------------------------------------------------------------- mixed-precision CG (SolveMixed)
// An fp32 CG recurrence corrected by fp64 reliable updates (kernels_mixed.hip has the loop and its kernels).  The host's side is cg_drive:
// an iteration is three launches, and behind every fourth iteration the three launches of an update are enqueued whether or not the device
// will want one -- they look at a device gate and return at their first instruction when it is closed, so the host decides nothing and the
// pipeline never drains.  The period is compiled in (kMixedUpdateEvery), not a knob: no knob may change a result.  The matrix is read as
// plain CSR in both precisions, so no compressed form, no placement draw and no deferred x update.
constexpr int kMixedUpdateEvery = 4;
static int cg_solve_mixed(CgRun& R, const float* e32, int* iteration, double* residual, int* reliableUpdates, double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f = cg_finalize_args(R, true, 0);
    if (!ws->ensure_mixed(n) || !cg_trace_columns(ws, 1, residualTrace, traceCapacity, f)) return MGCG_ERROR;
    if (R.elementsCount >= 8) R.cfg.periodRows = spmv_period(R.cusparse, R.rowOffsets, R.columnIndeces, n, 0, &R.cfg.maxRow);
    MixedRun M{};
    M.ws = ws; M.e32 = e32; M.rowOffsets = R.rowOffsets; M.columnIndeces = R.columnIndeces; M.n = n; M.nnz = R.elementsCount; M.x = R.x; M.r = R.r;
    M.xs = ws->mixedVecs; M.r32 = M.xs + ws->mixedStride; M.p32 = M.r32 + ws->mixedStride; M.Ap32 = M.p32 + ws->mixedStride;
    const bool refDots = dot_reference_order();
    // r = b - A x and the partial sums of r.r: the fp64 product of the start and of every update (gate: a device int, nonzero = skip)
    auto residual_product = [&](const int* gate) {
        SpmvArgs a = cg_spmv_args(R, R.x, R.r);
        a.b = R.b; a.partials = ws->partials; a.doneFlag = gate;
        int nP = launch_spmv_auto(s, EPI_RESIDUAL_DOT, a, R.cfg, nullptr);
        if (refDots) { launch_dot_serial(s, R.r, R.r, n, ws->partials, gate); nP = 1; }
        return nP;
    };
    if (R.rule == MGCG_RULE_SIMPLE) launch_fill(s, R.x, 0.0, n);                         // SimpleConjugateGradient.cu:53
    mixed_enqueue_start(M, f, residual_product(nullptr));
    bool ok = MGCG_HIP(hipGetLastError());
    long long hostIt = 0;
    ok = ok && cg_drive(R, "SolveMixed", [&] {
        if (!mixed_enqueue_iteration(M, f)) return false;
        if (++hostIt % kMixedUpdateEvery == 0) {                                         // behind iterations 3, 7, 11, ...: the device's it % 4 == 3
            mixed_enqueue_fold(M);
            mixed_enqueue_restart(M, f, residual_product(mixed_gate(M)));
        }
        return MGCG_HIP(hipGetLastError());
    });
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    MixedScalars h{};
    ok = ok && MGCG_HIP(hipMemcpy(&h, ws->mixedScalars, sizeof(h), hipMemcpyDeviceToHost));
    if (!ok) return MGCG_ERROR;
    if (reliableUpdates) *reliableUpdates = h.updates;
    return cg_return_one(R, "SolveMixed", f.traceCap, iteration, residual, residualTrace, "true residual", "",
                         "p.Ap is not finite and > 0, or the residual is not finite or beyond the fp32 range");
}

// ---------------------------------------------------------------- single-reduction CG (SolveSingleReduce, SolveSingleReduceParallel)
// Chronopoulos-Gear CG: the product in front of both sums, one reduction point per iteration (kernels_sreduce.hip has the loop and its pass).
// The host's side is cg_drive: a body is the product and the pass (two launches), on several ranks the product, the three sums, their one
// all-reduce and the pass.  The product is the plain loop's (cg_enqueue_product: halo exchange of the full-length buffer, which holds u here,
// launch_spmv_auto with the partial sums of w.u), so compression modes and automatic column tiles apply unchanged; the overlap schedule
// stays "in line", and the deferred x update and the placement draw do not apply.  R.Ap holds w, R.p u (full length), sVec s; the
// direction p takes the first library slot of the deferred x update's ring.  Without dinv the residual lives in the rows' slice of R.p
// while the loop runs and is copied into R.r at the end.
static int cg_solve_sreduce(CgRun& R, double* sVec, int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_sreduce()) return MGCG_ERROR;
    if (!ws->ensure_ring(2, n > 0 ? n : 1)) { set_error("SolveSingleReduce: no room on the device for the direction vector (%lld entries)", n); return MGCG_ERROR; }
    if (!cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    CgScalars* sc = ws->scalars;
    double* uLoc = R.p + R.offset;
    const SreduceRun P = { ws, R.x, ws->ring[1], sVec, R.r, uLoc, R.Ap, R.dinv, n, R.multi };

    // start: r = b - A x ; u = dinv r ; the partial sums of rr0 = r.r and gamma = r.u where body 0 looks for them ; the scalars
    bool ok = cg_enqueue_residual(R, R.p, R.r);
    double* rrPartials = sreduce_rr_partials(ws, 1);
    double* gPartials = R.dinv ? sreduce_gamma_partials(ws, 1) : nullptr;
    int nIn = ok ? launch_copy_dot(s, uLoc, R.r, R.dinv, n, rrPartials, gPartials, nullptr) : 0;
    if (ok && R.multi) ok = cg_share_sums(R, rrPartials, nIn, gPartials, nIn, R.dinv ? &sc->rrNew : &sc->rr, nullptr);   // rr0 for the relative rule, as cg_enqueue_init; {rrNew, rzNew} are adjacent
    if (ok) launch_init_scalars(s, rrPartials, gPartials, nIn, !R.multi, sc, ws->mirror);
    ok = ok && MGCG_HIP(hipGetLastError());

    ok = ok && cg_drive_bodies(R, "SolveSingleReduce", [&](int k) {
        int nDelta = 0;
        if (!cg_enqueue_product(R, R.p, &nDelta)) return false;                          // w = A u ; w.u
        if (R.multi) {
            sreduce_enqueue_sums(P, k, nDelta, nIn);
            if (!comm_allreduce_sum(R.comm, ws->sreduceScalars->red, R.dinv ? 3 : 2, s)) return false;
        }
        nIn = sreduce_enqueue_pass(P, f, k, nDelta, nIn);
        return true;
    });
    if (ok && !R.dinv) launch_copy(s, R.r, uLoc, n);                                     // the residual into the caller's r
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (!ok) return MGCG_ERROR;
    return cg_return_one(R, "SolveSingleReduce", f.traceCap, iteration, residual, residualTrace, "residual", "",
                         "w.u or its corrected form is not finite and > 0, or alpha or the residual is not finite");
}

// ---------------------------------------------------------------- MINRES (SolveMinres, SolveMinresParallel)
// Paige and Saunders' MINRES for (A - shift I) x = b, A symmetric of any inertia (include/MgcgGpu.h has the method, kernels_minres.hip the two
// passes).  The host's side is cg_drive: a body is the product and the two passes (three launches), on several ranks the product, a fold and an
// all-reduce of delta, pass A, a fold and an all-reduce of y.y, pass B.  The product is the plain loop's (cg_enqueue_product: halo exchange of
// the full-length buffer that holds v, launch_spmv_auto with the partial sums of v.q), so compression modes and automatic column tiles apply
// unchanged; the overlap schedule stays "in line", and the deferred x update and the placement draw do not apply.  The caller's p and r are the
// two full-length Lanczos buffers, rotated per body by pointer; w1Vec and w2Vec the two direction buffers, rotated the same way; R.Ap holds q.
// One more product behind the loop leaves the true residual b - (A - shift I) x in the first nLocal entries of the caller's r.
static int cg_solve_minres(CgRun& R, double* w1Vec, double* w2Vec, double shift, int* iteration, double* residual, double* trueResidual,
                           double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_minres() || !cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    MinresScalars* ms = ws->minresScalars;
    const int* done = &ws->scalars->done;
    double* const bufP = R.p; double* const bufR = R.r;                                  // the caller's two full-length buffers
    double* yyPartials = minres_yy_partials(ws);

    // start: t = b - A x through bufP ; r0 = t + shift x and v = r0 / || r0 || in the rows' slice of bufR ; r0.r0 in red[1] (several ranks:
    // all-reduced); bufP, which held x for the product, is body 0's vprev (not read there)
    bool ok = cg_enqueue_residual(R, bufP, R.Ap);
    if (ok) {
        const int nIn = minres_enqueue_residual(ws, R.Ap, R.x, bufR + R.offset, n, shift);
        if (R.multi) ok = cg_share_sums(R, yyPartials, nIn, nullptr, 0, &ms->red[1], nullptr);
        if (ok) minres_enqueue_start(ws, f, nIn, !R.multi, bufR + R.offset, n);
    }
    ok = ok && MGCG_HIP(hipGetLastError());

    double *v = bufR, *vprev = bufP, *w1 = w1Vec, *w2 = w2Vec;
    ok = ok && cg_drive_bodies(R, "SolveMinres", [&](int k) {
        int nDelta = 0;
        R.p = v;                                                                         // the buffer whose halo the product exchanges
        if (!cg_enqueue_product(R, v, &nDelta)) return false;                            // q = A v ; v.q
        const MinresRun P = { ws, R.x, v + R.offset, vprev + R.offset, w1, w2, R.Ap, n, shift, R.multi };
        if (R.multi && !cg_share_sums(R, ws->partials, nDelta, nullptr, 0, &ms->red[0], done)) return false;
        const int nYY = minres_enqueue_lanczos(P, k, nDelta);                            // y over vprev ; y.y
        if (R.multi && !cg_share_sums(R, yyPartials, nYY, nullptr, 0, &ms->red[1], done)) return false;
        minres_enqueue_update(P, f, k, nYY);                                             // w over w1 ; x ; vnext over y
        std::swap(v, vprev); std::swap(w1, w2);                                          // (vprev, v) := (v, vnext) ; (w1, w2) := (w2, w)
        return true;
    });
    R.p = bufP;
    // the closing product: the true residual t + shift x into the caller's r, whatever the parity of the rotation
    return cg_close_true_residual(R, ok, "SolveMinres", bufP, R.Ap, [&] { return minres_enqueue_residual(ws, R.Ap, R.x, bufR, n, shift); }, yyPartials, &ms->red[2],
                                  f.traceCap, iteration, residual, trueResidual, residualTrace, "",
                                  "the first residual is zero or not finite, or the rotation broke down (A - shift I singular on the Krylov space, or a value that is not finite)");
}

// ---------------------------------------------------------------- LSQR (MgcgSolveLsqr)
// Paige and Saunders' LSQR for min || A x - b ||_2 (+ damp^2 || x ||^2), A any CSR matrix of rows x columns, one rank (include/MgcgGpu.h has the
// method, kernels_lsqr.hip the passes).  The loop multiplies by two matrices of different shapes -- A, and A^T as the caller stored it -- so
// each has a description of its own (LsqrMatrix: kernel configuration, far band, analysed form), set up as cg_matrix_setup and CsrMV's
// rectangular path set one up; CgRun, which describes one square matrix, carries only what the host's side of the loop reads: the workspace
// and the stop rule.  Both products are launch_spmv_auto, so compression modes and the automatic column tiles apply to each matrix.
struct LsqrMatrix {
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    int elementsCount, rows, columns;
    SpmvConfig cfg; const DcsrMatrix* dcsr = nullptr;
};
static void lsqr_matrix_setup(MgcgSparse* h, LsqrMatrix& M)
{
    long long meanDistance = 0;
    M.cfg = cfg_of(h);
    if (M.elementsCount >= 8) M.cfg.periodRows = spmv_period(h, M.rowOffsets, M.columnIndeces, M.rows, 0, &M.cfg.maxRow, &meanDistance);
    M.dcsr = dcsr_lookup(h, M.elements, M.rowOffsets, M.columnIndeces, M.rows, M.elementsCount, 0, M.columns, meanDistance);
    if (meanDistance >= (1LL << 19) && M.columns >= (8LL << 19)) M.cfg.flags |= 16;     // gathers without locality: the stream form among the CSR kernels
    M.cfg.flags |= 8;                            // as the plain CG loop: the row-tile kernel may read the matrix with the non-temporal hint
}
// y = M x (b null) or y = b - M x; gate: a device int, nonzero = the product writes nothing
static void lsqr_enqueue_product(hipStream_t s, const LsqrMatrix& M, const double* x, double* y, const double* b, const int* gate)
{
    SpmvArgs a{};
    a.elements = M.elements; a.rowOffsets = M.rowOffsets; a.columnIndeces = M.columnIndeces; a.x = x; a.y = y;
    a.elementsCount = M.elementsCount; a.rowCount = M.rows; a.columnCount = M.columns;
    a.alpha = 1.0; a.beta = 0.0; a.b = b; a.doneFlag = gate;
    launch_spmv_auto(s, b ? EPI_RESIDUAL : EPI_AXPBY, a, M.cfg, M.dcsr);
}

static int lsqr_solve(CgRun& R, LsqrMatrix& A, LsqrMatrix& At, const LsqrRun& P, int* iteration, double* residual, double* residualNorm,
                      double* trueResidual, double* trueNormalResidual, double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const char* who = "MgcgSolveLsqr";
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f = cg_finalize_args(R, true, 0);
    if (!ws->ensure_lsqr() || !cg_trace_columns(ws, 1, residualTrace, traceCapacity, f)) return MGCG_ERROR;
    lsqr_matrix_setup(R.cusparse, A);
    lsqr_matrix_setup(R.cusparse, At);
    const int* done = &ws->scalars->done;

    // start: x = 0, uh = b, beta1 ; t = A^T uh ; vh = t / beta1, alpha1, g0
    lsqr_enqueue_start_beta(P);
    lsqr_enqueue_product(s, At, P.uh, P.t, nullptr, nullptr);
    lsqr_enqueue_start_alpha(P, f);
    bool ok = MGCG_HIP(hipGetLastError());

    ok = ok && cg_drive_bodies(R, who, [&](int k) {
        lsqr_enqueue_product(s, A, P.vh, P.q, nullptr, done);                            // q = A vh
        const int nUU = lsqr_enqueue_u(P, k);                                            // uh ; uh.uh
        lsqr_enqueue_product(s, At, P.uh, P.t, nullptr, done);                           // t = A^T uh
        lsqr_enqueue_v(P, f, k, nUU);                                                    // w ; x ; vh ; vh.vh ; the scalars
        return true;
    });
    // the two closing products: r = b - A x over uh, t = A^T r - damp^2 x over t, and their 2-norms
    LsqrScalars h{};
    if (ok) {
        lsqr_enqueue_product(s, A, P.x, P.uh, P.b, nullptr);
        const int nR = lsqr_enqueue_close_residual(P);
        lsqr_enqueue_product(s, At, P.uh, P.t, nullptr, nullptr);
        const int nT = lsqr_enqueue_close_normal(P);
        launch_reduce2_to(s, lsqr_uu_partials(ws), nR, &ws->lsqrScalars->red[0], lsqr_vv_partials(ws), nT, &ws->lsqrScalars->red[1], nullptr);
        ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&h, ws->lsqrScalars, sizeof(h), hipMemcpyDeviceToHost, s));
    }
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (!ok) return MGCG_ERROR;
    if (residualNorm) *residualNorm = h.resNorm;
    if (trueResidual) *trueResidual = std::sqrt(h.red[0]);
    if (trueNormalResidual) *trueNormalResidual = std::sqrt(h.red[1]);
    const char* nonfinite = h.note == 1 ? "beta_1 = || b || is zero or not finite"
                          : h.note == 2 ? "alpha_1 = || A^T b || / beta_1 is zero or not finite (a nonzero b is orthogonal to the range of A)"
                          : h.note == 3 ? "g_0 = alpha_1 beta_1 has a square that is zero or not finite"
                          : "a scalar of the bidiagonalisation or of the rotation is not finite";
    return cg_return_one(R, who, f.traceCap, iteration, residual, residualTrace, "normal residual", "", nonfinite);
}

// ---------------------------------------------------------------- LOBPCG (MgcgSolveLobpcg, MgcgSolveLobpcgMg)
// The k extreme eigenpairs of a symmetric CSR matrix (include/MgcgGpu.h has the method, kernels_lobpcg.hip the passes and the dense step), one
// rank.  The matrix is read as plain CSR by the block product, so no matrix set-up; the host's side is cg_drive.  A body is the residual pass,
// with a hierarchy k cycles W_j = M^-1 R_j, and the rest (lob_enqueue_rest); CgRun carries what the host's side of the loop reads.
static int lob_solve(CgRun& R, LobRun& P, MgcgMg* mg, const char* who, int* iteration, double theta[], double residual[], double trueResidual[],
                     int status[], int* restarts, double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const int k = P.k;
    const int cap = (residualTrace && traceCapacity > 0) ? traceCapacity : 0;
    // everything the call allocates, before anything is enqueued
    if (!ws->ensure_lobpcg() || (cap && !ws->ensure_trace(k * cap))) return MGCG_ERROR;
    P.trace = cap ? ws->trace : nullptr; P.traceCap = cap;
    const int* done = &ws->scalars->done;
    hipLaunchKernelGGL(clear_done_kernel, dim3(1), dim3(1), 0, s, ws->scalars);
    bool ok = lob_enqueue_start(P);
    ok = ok && cg_drive_bodies(R, who, [&](int body) {
        const int nR = lob_enqueue_residual(P);
        for (int j = 0; mg && j < k; ++j)
            if (!mg_apply(mg, P.Rv + j * P.ld, P.W + j * P.ld, done)) return false;          // W_j = M^-1 R_j
        return lob_enqueue_rest(P, body, nR);
    });
    ok = ok && lob_enqueue_close(P);
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    LobResult h{};
    ok = ok && lob_read_results(ws, k, &h);
    if (!ok) return MGCG_ERROR;
    const bool startFailed = h.failWhich == 1 || h.failWhich == 5;
    if (iteration) *iteration = startFailed ? -1 : h.iteration;      // the last body that was judged: none when the start broke down
    if (restarts) *restarts = h.restarts;
    int nTrace[kBlockMaxK];
    for (int j = 0; j < k; ++j) {
        nTrace[j] = startFailed ? 0 : h.iteration + 1;
        if (theta) theta[j] = h.theta[j];
        if (trueResidual) trueResidual[j] = startFailed ? NAN : h.trueResidual[j];
    }
    const int worst = cg_return_columns(ws, k, nullptr, h.residual, h.status, nTrace, cap, nullptr, residual, status, residualTrace, traceCapacity, &ok);
    if (h.failWhich) {
        static const char* const names[] = { "", "the first factorisation, of X0^T X0 (dependent or zero start columns)", "the factorisation of W^T W (a zero or dependent column of W)",
                                             "the factorisation of the basis [X W]^T [X W]", "the Ritz values: one is not finite", "the Ritz values of the start block: one is not finite" };
        set_error("%s: breakdown in %s: pivot %d is not finite and > 0 (body %d); X, AX and theta keep the last completed body", who, names[h.failWhich], h.failPivot, h.iteration);
    } else cg_columns_message(who, worst, "a residual is not finite", R.maxIt);
    return ok ? worst : MGCG_ERROR;
}

// ---------------------------------------------------------------- BiCGStab (SolveBicgstab*, SolveBicgstabJacobi*)
// Van der Vorst's BiCGStab for A x = b, A any CSR matrix, right-preconditioned with M = I or M = diag(A) (R.dinv) (include/MgcgGpu.h has the
// method, kernels_bicgstab.hip the passes).  The host's side is cg_drive: a body is two products and four passes (six launches), on several ranks
// with a fold and an all-reduce behind each of its three reduction points: sigma, {theta, tau}, {rr, rhon}.  Both products are the plain loop's
// (cg_enqueue_product: halo exchange of the full-length buffer in line, launch_spmv_auto with the partial sums of w.Ap), so compression modes and
// automatic column tiles apply unchanged; the overlap schedule stays "in line", and the deferred x update and the placement draw do not apply.
// The caller's p and s are the two full-length buffers the products gather from: phat and shat, which without a diagonal are p and s themselves.
// With a diagonal s is written over r and p lives in the caller's Ap vector.  One more product behind the loop leaves the true residual b - A x in
// the caller's r.
static int cg_solve_bicgstab(CgRun& R, const char* who, double* vVec, double* sVec, double* tVec, double* rhatVec, int* iteration, double* residual, double* trueResidual,
                             double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_bicgstab() || !cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    BicgstabScalars* bs = ws->bicgstabScalars;
    const int* done = &ws->scalars->done;
    double* const bufP = R.p; double* const bufS = sVec; double* const work = R.Ap;      // the two full-length buffers; the caller's Ap
    BicgstabRun P{};
    P.ws = ws; P.x = R.x; P.r = R.r; P.v = vVec; P.t = tVec; P.rhat = rhatVec; P.dinv = R.dinv; P.n = n; P.given = R.multi;
    P.phat = bufP + R.offset; P.shat = bufS + R.offset;
    const bool hatted = R.dinv || R.mg;                                                  // phat and shat are vectors of their own
    P.p = hatted ? work : P.phat; P.s = hatted ? R.r : P.shat; P.stored = R.mg != nullptr;
    // The V-cycle form: zhat = M^-1 z into the buffer the next product gathers from, gated on the live stop flag as in cg_solve_pminres.  A
    // cycle writes nothing but its output and the hierarchy's own iterates, so one enqueued behind the stop is skipped whole, and one behind a
    // breakdown of pass S writes shat only, which nothing reads afterwards.
    auto cycle = [&](const double* z, double* zhat) { return !R.mg || mg_apply(R.mg, z, zhat, done); };

    // start: r = b - A x through bufP ; rhat = r ; p = r ; phat = dinv r (the V-cycle form: body 0's first cycle) ; rho = rr0 = r.r
    bool ok = cg_enqueue_residual(R, bufP, R.r);
    if (ok) {
        const int nRr = bicgstab_enqueue_start(P);
        if (R.multi) ok = cg_share_sums(R, bicgstab_rr_partials(ws), nRr, nullptr, 0, &bs->red[3], nullptr);
        if (ok) bicgstab_enqueue_init(ws, f, nRr, !R.multi);
    }
    ok = ok && MGCG_HIP(hipGetLastError());

    ok = ok && cg_drive_bodies(R, who, [&](int k) {
        int nSigma = 0, nTheta = 0;
        R.p = bufP; R.Ap = P.v;
        if (!cycle(P.p, P.phat)) return false;                                           // the V-cycle form: phat = M^-1 p
        if (!cg_enqueue_product(R, bufP, &nSigma, P.rhat)) return false;                 // v = A phat ; sigma = rhat.v
        if (R.multi && !cg_share_sums(R, ws->partials, nSigma, nullptr, 0, &bs->red[0], done)) return false;
        bicgstab_enqueue_s(P, f, k, nSigma);                                             // alpha ; s ; shat
        R.p = bufS; R.Ap = P.t;
        if (!cycle(P.s, P.shat)) return false;                                           // the V-cycle form: shat = M^-1 s
        if (!cg_enqueue_product(R, bufS, &nTheta, P.s)) return false;                    // t = A shat ; theta = s.t
        const int nTau = bicgstab_enqueue_tau(P);                                        // tau = t.t
        if (R.multi && !cg_share_sums(R, ws->partials, nTheta, bicgstab_tau_partials(ws), nTau, &bs->red[1], done)) return false;
        const int nRr = bicgstab_enqueue_x(P, f, k, nTheta, nTau);                       // omega ; x ; r ; rr, rhon
        if (R.multi && !cg_share_sums(R, bicgstab_rr_partials(ws), nRr, bicgstab_rho_partials(ws), nRr, &bs->red[3], done)) return false;
        bicgstab_enqueue_p(P, f, k, nRr);                                                // the stop decision ; beta ; p ; phat
        return true;
    });
    R.p = bufP; R.Ap = work;
    // the closing product: the true residual into the caller's r
    return cg_close_true_residual(R, ok, who, bufP, R.r, [&] { return launch_dot_partials(s, R.r, R.r, n, bicgstab_rr_partials(ws)); }, bicgstab_rr_partials(ws), &bs->red[5],
                                  f.traceCap, iteration, residual, trueResidual, residualTrace, "",
                                  "the first residual is zero or not finite, or the recurrence broke down (rhat.v, omega or rhat.r zero, or a value that is not finite)");
}

// ---------------------------------------------------------------- BiCGStab(l) (SolveBicgstabL, SolveBicgstabLJacobi)
// Sleijpen and Fokkema's BiCGStab(l) for A x = b, A any CSR matrix, l = 1 .. 4, right-preconditioned with M = I or M = diag(A) (R.dinv), one
// rank (include/MgcgGpu.h has the method, kernels_bicgstabl.hip the passes).  The host's side is cg_drive: a body is 2 l products and 2 l + 2
// passes (4 l + 2 launches); a body that the device ends in front of a step (r_0 converged) is enqueued whole, its later launches return.  Every product is the plain loop's (cg_enqueue_product with w = rt, output and gather vector switched per product),
// so compression modes and automatic column tiles apply unchanged; the deferred x update and the placement draw do not apply.  The caller's r is
// r_0, its p u_0 and its Ap u_l; `work` holds r_1 .. r_l, u_1 .. u_{l-1}, rt and -- with a diagonal -- the one gather buffer, `stride` entries
// apart.  Without a diagonal the products gather from u_j and r_j themselves.  One more product behind the loop leaves the true residual b - A x
// in the caller's r.
static int bicgstabl_slices(int ell, bool jacobi) { return 2 * ell + (jacobi ? 1 : 0); }
static int cg_solve_bicgstabl(CgRun& R, const char* who, int ell, double* work, int* iteration, double* residual, double* trueResidual,
                              double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_bicgstabl() || !cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    double* const bufP = R.p; double* const bufAp = R.Ap;
    const long long stride = cg_work_stride(R.count);
    BicgstablRun P{};
    P.ws = ws; P.ell = ell; P.x = R.x; P.dinv = R.dinv; P.n = n;
    P.r[0] = R.r; P.u[0] = bufP; P.u[ell] = bufAp;
    for (int j = 1; j <= ell; ++j) P.r[j] = work + (j - 1) * stride;
    for (int j = 1; j < ell; ++j) P.u[j] = work + (ell + j - 1) * stride;
    P.rt = work + (2 * ell - 1) * stride;
    P.gather = R.dinv ? work + 2 * ell * stride : nullptr;

    // start: r_0 = b - A x through bufP ; rt = r_0 ; u_0 = r_0 ; gather = dinv r_0 ; rho = rr0 = r_0.r_0
    bool ok = cg_enqueue_residual(R, bufP, R.r);
    if (ok) {
        BicgstabRun S{};
        S.ws = ws; S.r = R.r; S.rhat = P.rt; S.p = P.u[0]; S.phat = P.gather; S.dinv = R.dinv; S.n = n;
        bicgstabl_enqueue_init(ws, f, bicgstab_enqueue_start(S));
    }
    ok = ok && MGCG_HIP(hipGetLastError());

    // out = A hat(v) with the partial sums of rt.out
    auto product = [&](double* v, double* out, int* nSums) {
        double* from = P.gather ? P.gather : v;
        R.p = from; R.Ap = out;
        return cg_enqueue_product(R, from, nSums, P.rt);
    };
    ok = ok && cg_drive_bodies(R, who, [&](int k) {
        int nSums = 0, nRrStep = 0;
        for (int j = 0; j < ell; ++j) {
            if (j > 0) bicgstabl_enqueue_u(P, f, k, j, nSums, nRrStep);                  // the stop test on r_0 ; beta ; u_0 .. u_j ; hat(u_j)
            if (!product(P.u[j], P.u[j + 1], &nSums)) return false;                      // u_{j+1} = A hat(u_j) ; sigma = rt.u_{j+1}
            nRrStep = bicgstabl_enqueue_r(P, f, k, j, nSums);                            // alpha ; r_0 .. r_j ; x ; hat(r_j) ; r_0.r_0
            if (!product(P.r[j], P.r[j + 1], &nSums)) return false;                      // r_{j+1} = A hat(r_j) ; rt.r_{j+1}
        }
        const int nGram = bicgstabl_enqueue_gram(P);                                     // Z
        const int nRr = bicgstabl_enqueue_combine(P, f, k, nGram);                       // gamma ; u_0 ; x ; r_0 ; rr, rhon
        bicgstabl_enqueue_p(P, f, k, nRr);                                               // the stop decision ; beta ; u_0 ; hat(u_0)
        return true;
    });
    R.p = bufP; R.Ap = bufAp;
    // the closing product: the true residual into the caller's r
    return cg_close_true_residual(R, ok, who, bufP, R.r, [&] { return launch_dot_partials(s, R.r, R.r, n, bicgstab_rr_partials(ws)); }, bicgstab_rr_partials(ws), &ws->bicgstablScalars->red,
                                  f.traceCap, iteration, residual, trueResidual, residualTrace, "",
                                  "the first residual is zero or not finite, or the recurrence broke down (rt.u_{j+1}, omega or rt.r_0 zero, or a value that is not finite)");
}

// ---------------------------------------------------------------- GMRES(m) (SolveGmres, SolveGmresJacobi, SolveGmresMg)
// Restarted GMRES for A x = b, A any CSR matrix, 1 <= m <= kGmresMaxM, right-preconditioned with M = I, M = diag(A) (R.dinv) or a V-cycle (R.mg), one rank
// (include/MgcgGpu.h has the method, kernels_gmres.hip the passes).  The host's side is cg_drive: an iteration is one Arnoldi step -- the
// product and the passes of gmres_enqueue_step -- and in front of every m-th the close and the restart.  Every product is the plain loop's
// (cg_enqueue_product, gather vector switched per step), so compression modes and automatic column tiles apply unchanged; the deferred x
// update and the placement draw do not apply.  The caller's r holds b - A x at the start and at every restart, its Ap is w, its p the
// full-length buffer the residual products gather x from; `work` holds v_0 .. v_m and -- with a diagonal -- the one gather buffer, `stride`
// entries apart.  The close is enqueued once more behind the loop: it applies the columns of the cycle that the stop, the cap or a breakdown
// cut short, and does nothing when a close in front of a restart that was enqueued behind the stop has done so already.  One more product
// leaves the true residual b - A x in the caller's r.
// The flexible form (SolveGmresMg, R.mg): behind v_0 .. v_m `work` holds z_0 .. z_{m-1}.  In front of step k's product a cycle writes
// z_j = M^-1 v_j straight into its slice, the product gathers from that slice, and the close adds sum y_i z_i (gmres_enqueue_close with
// P.Z).  The cycle and the product are gated on the live stop flag, which pass N alone raises and nobody writes while they run; a cycle
// enqueued behind a stop returns at the gate and leaves its slice unwritten, and the close -- not gated, keyed on cols -- reads columns
// below cols only, each of which a cycle that ran in front of the stop has written.  A cycle writes its slice and the hierarchy's own
// iterates, never x, V, w or a scalar of the loop.
static int gmres_slices(int m, bool jacobi, bool flexible) { return flexible ? 2 * m + 1 : m + 1 + (jacobi ? 1 : 0); }
static int cg_solve_gmres(CgRun& R, const char* who, int m, int orth, double* work, int* iteration, double* residual, double* trueResidual,
                          double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_gmres() || !cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    const int* done = &ws->scalars->done;
    double* const bufP = R.p; double* const bufAp = R.Ap;
    const long long stride = cg_work_stride(R.count);
    GmresRun P{};
    P.ws = ws; P.m = m; P.orth = orth; P.x = R.x; P.r = R.r; P.w = bufAp; P.V = work; P.dinv = R.dinv; P.stride = stride; P.n = n;
    P.gather = R.dinv ? work + (m + 1) * stride : nullptr;
    P.Z = R.mg ? work + (m + 1) * stride : nullptr;

    // r = b - A x through bufP ; beta^2 = r.r ; v_0 = r / beta ; gather = dinv v_0 ; g_0 = beta for step k.  The start also sets the scalars.
    auto restart = [&](int k, bool first) {
        if (!cg_enqueue_residual(R, bufP, R.r, first ? nullptr : done)) return false;
        const int nRr = launch_dot_partials(s, R.r, R.r, n, gmres_rr_partials(ws));
        if (first) gmres_enqueue_init(P, f, nRr);
        gmres_enqueue_restart(P, f, k, nRr, first);
        return true;
    };
    bool ok = restart(0, true) && MGCG_HIP(hipGetLastError());

    ok = ok && cg_drive_bodies(R, who, [&](int k) {
        const int j = k % m;
        if (j == 0 && k > 0) {                                                           // y ; x += hat(V y) ; the next cycle's r, v_0
            gmres_enqueue_close(P);
            if (!restart(k, false)) return false;
        }
        double* from = P.Z ? P.Z + j * stride : P.gather ? P.gather : P.V + j * stride;
        int nSums = 0;
        if (P.Z && !mg_apply(R.mg, P.V + j * stride, from, done)) return false;          // the flexible form: z_j = M^-1 v_j
        R.p = from; R.Ap = P.w;
        if (!cg_enqueue_product(R, from, &nSums)) return false;                          // w = A hat(v_j) (the flexible form: w = A z_j)
        gmres_enqueue_step(P, f, k, j);                                                  // h ; w ; the rotations ; the stop decision ; v_{j+1}
        return true;
    });
    R.p = bufP; R.Ap = bufAp;
    if (ok) gmres_enqueue_close(P);                                                      // the columns of the cycle that was cut short
    // the closing product: the true residual into the caller's r
    return cg_close_true_residual(R, ok, who, bufP, R.r, [&] { return launch_dot_partials(s, R.r, R.r, n, gmres_rr_partials(ws)); }, gmres_rr_partials(ws), &ws->gmresScalars->red,
                                  f.traceCap, iteration, residual, trueResidual, residualTrace, "",
                                  "the first residual is zero or not finite, or an Arnoldi step left no next direction and no column (A singular on the Krylov space, or a value that is not finite)");
}

// ---------------------------------------------------------------- preconditioned MINRES (SolveMinresJacobi, SolveMinresJacobiParallel, SolveMinresMg)
// MINRES with a symmetric positive definite preconditioner M (include/MgcgGpu.h has the method, kernels_pminres.hip the two passes): R.dinv --
// z = dinv r formed per element inside the passes -- or R.mg with R.z, the V-cycle enqueued between them with one dot launch for r.z (one rank).
// The host's side is cg_drive, and the product is the plain loop's, as in cg_solve_minres.  A body on several ranks (Jacobi only): the product, a
// fold and ONE all-reduce of the adjacent pair {v.q, v.v}, pass A, a fold and an all-reduce of r.z, pass B: two all-reduces, as the plain loop.
// R.p holds v, the one full-length buffer (pass B writes the next v over it in place); the caller's r and r1Vec are the two residual buffers,
// rotated per body by pointer; w1Vec and w2Vec the two direction buffers, rotated the same way; R.Ap holds q.  One more product behind the loop
// leaves the true residual b - (A - shift I) x in the caller's r, whatever the parity of the rotation.
static int cg_solve_pminres(CgRun& R, const char* who, double* r1Vec, double* w1Vec, double* w2Vec, double shift, int* iteration, double* residual, double* trueResidual,
                            double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    // everything the call allocates, before anything is enqueued
    FinalizeArgs f;
    if (!ws->ensure_minres() || !cg_variant_begin(R, 0, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    MinresScalars* ms = ws->minresScalars;
    const int* done = &ws->scalars->done;
    double* const bufR = R.r;                                                            // the caller's r
    double* vLoc = R.p + R.offset;
    double* rzPartials = pminres_rz_partials(ws);

    // z = M^-1 r into R.z and the partial sums of r.z (the V-cycle form)
    auto cycle = [&](const double* r, const int* gate, int* nRz) {
        if (!mg_apply(R.mg, r, R.z, gate)) return false;
        *nRz = launch_dot_partials(s, r, R.z, n, rzPartials);
        return true;
    };

    // start: t = b - A x through the buffer of v, into R.Ap ; r2 = t + shift x in the caller's r ; bz = r2 . M^-1 r2 ; v = M^-1 r2 / sqrt(bz) ; v.v
    int nRz = 0, nVv = 0;
    bool ok = cg_enqueue_residual(R, R.p, R.Ap);
    if (ok) nRz = pminres_enqueue_residual(ws, R.Ap, R.x, bufR, R.dinv, n, shift);
    if (ok && R.mg) ok = cycle(bufR, nullptr, &nRz);
    if (ok && R.multi) ok = cg_share_sums(R, rzPartials, nRz, nullptr, 0, &ms->red[3], nullptr);
    if (ok) nVv = pminres_enqueue_start(ws, f, nRz, !R.multi, vLoc, bufR, R.dinv, R.z, n);
    ok = ok && MGCG_HIP(hipGetLastError());

    double *r2 = bufR, *r1 = r1Vec, *w1 = w1Vec, *w2 = w2Vec;
    ok = ok && cg_drive_bodies(R, who, [&](int k) {
        int nVq = 0;
        if (!cg_enqueue_product(R, R.p, &nVq)) return false;                             // q = A v ; v.q
        const PminresRun P = { ws, R.x, vLoc, r1, w1, r2, w2, R.Ap, R.dinv, R.z, n, shift, R.multi };
        if (R.multi && !cg_share_sums(R, ws->partials, nVq, pminres_vv_partials(ws), nVv, &ms->red[0], done)) return false;   // {v.q, v.v}: one all-reduce of two doubles
        int nZ = pminres_enqueue_lanczos(P, k, nVq, nVv);                                // rn over r1 ; Jacobi: rn.z
        if (R.mg && !cycle(r1, done, &nZ)) return false;                                 // z = M^-1 rn ; rn.z
        if (R.multi && !cg_share_sums(R, rzPartials, nZ, nullptr, 0, &ms->red[3], done)) return false;
        nVv = pminres_enqueue_update(P, f, k, nZ);                                       // w over w1 ; x ; the next v in place ; v.v
        std::swap(r1, r2); std::swap(w1, w2);                                            // (r1, r2) := (r2, rn) ; (w1, w2) := (w2, w)
        return true;
    });
    // the closing product: the true residual into the caller's r
    double bz = 0.0;
    const int status = cg_close_true_residual(R, ok, who, R.p, R.Ap, [&] { return minres_enqueue_residual(ws, R.Ap, R.x, bufR, n, shift); }, minres_yy_partials(ws), &ms->red[2],
                                              f.traceCap, iteration, residual, trueResidual, residualTrace, " in the M^-1 norm",
                                              "the first residual is zero or not finite, r . M^-1 r is negative or not finite (a preconditioner that is not positive definite), or the rotation broke down (A - shift I singular on the Krylov space, or a value that is not finite)",
                                              [&] { return MGCG_HIP(hipMemcpyAsync(&bz, &ms->red[4], sizeof(double), hipMemcpyDeviceToHost, s)); });
    if (status != MGCG_ERROR && ws->mirror->status == MGCG_NONFINITE && ws->mirror->iteration == 0 && bz < 0.0)
        set_error("%s: stopped at iteration 0: the preconditioner is not positive definite (r . M^-1 r = %g for the first residual)", who, bz);
    return status;
}

// ---------------------------------------------------------------- Chebyshev-preconditioned CG (SolveChebyshev, SolveChebyshevParallel)
// SolveJacobi's loop with z = p_m(D^-1 A) D^-1 r (kernels_cheb.hip has the method and the passes): the polynomial costs m - 1 products and no
// global sum.  The host's side is cg_drive.  One iteration on one rank is m + 3 launches: the loop's product (cg_enqueue_product, so
// compression modes and automatic column tiles apply to it), the fused first pass, m - 1 steps, the finalisation and the preconditioned
// loop's x / p update.  Several ranks add a reduce and an all-reduce of p.Ap in front of the first pass and one reduce with ONE all-reduce
// of {r.r, r.z} behind the polynomial (CgUpdate::PrecondRanks' pair), and exchange the halo of z in line before every step; the overlap
// schedule, the deferred x update and the placement draw do not apply.  The steps read the matrix as plain CSR whatever the handle's
// compression mode (launch_spmv, not launch_spmv_auto): the lossless forms would give the same bits.
struct ChebPlan { int m; double it; double c1[16], c2[16]; };      // c1[j], c2[j]: step j = 1 .. m - 1

// The coefficients, once per call, in the order include/MgcgGpu.h states (this file is built without contraction, as the kernels are).
static ChebPlan cheb_plan(int degree, double lmin, double lmax)
{
    ChebPlan c{};
    c.m = degree;
    const double theta = (lmax + lmin) * 0.5, delta = (lmax - lmin) * 0.5, sigma = theta / delta;
    double rho = 1.0 / sigma;
    c.it = 1.0 / theta;
    for (int j = 1; j < degree; ++j) {
        const double next = 1.0 / (2.0 * sigma - rho);
        c.c1[j] = next * rho; c.c2[j] = (2.0 * next) / delta;
        rho = next;
    }
    return c;
}

// Steps 1 .. m - 1 behind the first pass, which left z in zA's rows: each gathers one full-length buffer and writes the rows of the other.
// *zFinal: the buffer that holds z afterwards; *nZ: the number of r.z partial sums the last step left in ws->partials (untouched at m = 1).
static bool cheb_enqueue_steps(CgRun& R, const ChebPlan& c, double* zA, double* zB, double* d, const int* done, double** zFinal, int* nZ)
{
    hipStream_t s = R.ws->stream;
    double *in = zA, *out = zB;
    for (int j = 1; j < c.m; ++j) {
        if (!halo_exchange(R.comm, R.halo, in, s)) return false;
        SpmvArgs a = cg_spmv_args(R, in, out + R.offset);
        a.w = in + R.offset; a.b = R.r; a.d = d; a.c1 = c.c1[j]; a.c2 = c.c2[j];
        a.dinv = R.dinv; a.dinvUniform = R.dinv ? 0 : 1; a.dinvScalar = 1.0;             // no diagonal: t = 1 * res, the same bits
        a.partials = R.ws->partials; a.doneFlag = done;
        const bool last = j == c.m - 1;
        const int n = launch_spmv(s, last ? EPI_CHEBYSHEV_DOT : EPI_CHEBYSHEV, a, R.cfg);
        if (last) *nZ = n;
        double* t = in; in = out; out = t;
    }
    *zFinal = in;
    if (c.m > 1 && dot_reference_order()) { launch_dot_serial(s, R.r, in + R.offset, R.nLocal, R.ws->partials, done); *nZ = 1; }   // validation mode: r.z once more, in the reference's order
    return true;
}

static int cg_solve_chebyshev(CgRun& R, const ChebPlan& c, double* zA, double* zB, double* dVec, int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    FinalizeArgs f;
    if (!cg_variant_begin(R, 2, residualTrace, traceCapacity, &f)) return MGCG_ERROR;
    CgScalars* sc = ws->scalars;
    const int* done = &sc->done;
    double* pLoc = R.p + R.offset;
    // the first pass's partial sums of r.r (and, at degree 1, of r.z) take the third region of the buffer, as the r update's do; the last
    // step's partial sums of r.z take the first, behind the product's of p.Ap, which the first pass has consumed by then
    double* rrPartials = ws->partials + 2 * kMaxPartials;
    double* rzFirst = rrPartials + kMaxPartials / 2;
    const bool one = c.m == 1;
    const double* rzPartials = one ? rzFirst : ws->partials;

    // start: r = b - A x ; z = M r ; r.r and r.z ; the scalars (an r.z that is not > 0 stops the loop here) ; p = z
    bool ok = cg_enqueue_residual(R, R.p, R.r);
    if (ok) {
        const int nrr = launch_cheb_start(s, R.r, R.dinv, dVec, zA + R.offset, n, c.it, rrPartials, rzFirst, one);
        int nz = nrr;
        double* zFin = zA;
        ok = cheb_enqueue_steps(R, c, zA, zB, dVec, nullptr, &zFin, &nz);
        if (ok && R.multi) ok = cg_share_sums(R, rrPartials, nrr, rzPartials, nz, &sc->rrNew, nullptr);
        if (ok) {
            launch_cheb_init_scalars(s, rrPartials, nrr, rzPartials, nz, !R.multi, f);
            launch_copy(s, pLoc, zFin + R.offset, n);
        }
    }
    ok = ok && MGCG_HIP(hipGetLastError());

    ok = ok && cg_drive(R, "SolveChebyshev", [&] {
        int nPAp = 0;
        if (!cg_enqueue_product(R, R.p, &nPAp)) return false;                            // Ap = A p ; p.Ap
        if (R.multi && !cg_share_sums(R, ws->partials, nPAp, nullptr, 0, &sc->pAp, done)) return false;
        const int nrr = launch_cheb_first(s, f, R.r, R.Ap, R.dinv, dVec, zA + R.offset, n, c.it, rrPartials, rzFirst, one,
                                          R.multi ? nullptr : ws->partials, R.multi ? 0 : nPAp);
        int nz = nrr;
        double* zFin = zA;
        if (!cheb_enqueue_steps(R, c, zA, zB, dVec, done, &zFin, &nz)) return false;
        if (R.multi && !cg_share_sums(R, rrPartials, nrr, rzPartials, nz, &sc->rrNew, done)) return false;   // {rrNew, rzNew} are adjacent in CgScalars: one all-reduce
        launch_cheb_finalize(s, rrPartials, nrr, rzPartials, nz, !R.multi, f);
        launch_update_xp(s, sc, R.x, pLoc, zFin + R.offset, n);                          // x += alpha p ; p = z + beta p
        return MGCG_HIP(hipGetLastError());
    });
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (!ok) return MGCG_ERROR;
    return cg_return_one(R, "SolveChebyshev", f.traceCap, iteration, residual, residualTrace, "residual", "",
                         "p.Ap or r.z is not finite and > 0 (an upper bound below the spectrum makes the polynomial indefinite), or the residual is not finite");
}

// ---------------------------------------------------------------- shared-subspace block CG (SolveBlockKrylov)
// k right-hand sides in one block Krylov space (kernels_bkrylov.hip has the method and the kernels).  The matrix is read as plain CSR by the
// block product, so no matrix set-up, no placement draw and no deferred x update; the host's side is cg_drive.  R.p, R.r and R.Ap hold S, Q, T.
static int cg_solve_bkrylov(CgRun& R, int k, int* iteration, double residual[], int status[], double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    hipStream_t s = ws->stream;
    const long long n = R.nLocal;
    FinalizeArgs f = cg_finalize_args(R, true, 0);
    if (!ws->ensure_bkrylov() || !cg_trace_columns(ws, k, residualTrace, traceCapacity, f)) return MGCG_ERROR;
    const BkRun B = { ws, R.elements, R.rowOffsets, R.columnIndeces, n, k, R.x, R.b, R.p, R.r, R.Ap };
    hipLaunchKernelGGL(clear_done_kernel, dim3(1), dim3(1), 0, s, ws->scalars);
    if (R.rule == MGCG_RULE_SIMPLE) launch_fill(s, R.x, 0.0, (long long)k * n);       // SimpleConjugateGradient.cu:53, per column (as SolveBlockEx)
    bool ok = bk_enqueue_start(B);
    ok = ok && cg_drive(R, "SolveBlockKrylov", [&] { return bk_enqueue_iteration(B, f); });
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    BkResult h{};
    ok = ok && bk_read_results(ws, k, &h);
    if (!ok) return MGCG_ERROR;
    if (iteration) *iteration = h.iteration;
    int nTrace[kBlockMaxK];                            // a breakdown leaves no entry for its iteration; one in the first factorisation, none at all
    for (int j = 0; j < k; ++j) nTrace[j] = h.failWhich == 1 ? 0 : h.iteration + (h.failWhich ? 0 : 1);
    const int worst = cg_return_columns(ws, k, nullptr, h.residual, h.status, nTrace, f.traceCap, nullptr, residual, status, residualTrace, traceCapacity, &ok);
    if (h.failWhich) {
        static const char* const names[] = { "", "the first factorisation, of R0^T R0 (dependent or zero initial residual columns)", "the factorisation of S^T A S (is the matrix positive definite?)",
                                             "the factorisation of W^T W" };
        set_error("SolveBlockKrylov: breakdown in %s: pivot %d is not finite and > 0 (iteration %d); x keeps the last completed iterate -- fall back to SolveBlockEx",
                  names[h.failWhich], h.failPivot, h.iteration);
    } else cg_columns_message("SolveBlockKrylov", worst, "the residual of a column is not finite", R.maxIt);
    return ok ? worst : MGCG_ERROR;
}

// ---------------------------------------------------------------- block CG (SolveBlockEx)
// k independent CG recurrences that share the matrix pass (kernels_block.hip has the layout and the kernels).  The matrix is read as plain CSR by
// the block product, so no matrix set-up, no placement draw and no deferred x update; the host's side is cg_drive_on with the snapshot of the loop's own stop flag.
static int cg_solve_block(CgRun& R, int k, int iteration[], double residual[], int status[], double* residualTrace, int traceCapacity)
{
    Workspace* ws = R.ws;
    FinalizeArgs f = cg_finalize_args(R, true, 0);
    if (!ws->ensure_block() || !cg_trace_columns(ws, k, residualTrace, traceCapacity, f)) return MGCG_ERROR;
    const BlockRun B = { ws, R.elements, R.rowOffsets, R.columnIndeces, R.nLocal, k, R.rule, R.x, R.b, R.Ap, R.p, R.r };
    bool ok = block_enqueue_start(B);
    ok = ok && cg_drive_on(R, "SolveBlockEx", [&] { return block_enqueue_iteration(B, f); }, [&](volatile int* slot) { block_enqueue_snapshot(ws, slot); });
    ok = MGCG_HIP(hipStreamSynchronize(ws->stream)) && ok;
    BlockResult h;
    ok = ok && block_read_results(ws, &h);
    if (!ok) return MGCG_ERROR;
    const int worst = cg_return_columns(ws, k, h.iteration, h.residual, h.status, nullptr, f.traceCap, iteration, residual, status, residualTrace, traceCapacity, &ok);
    if (ok) cg_columns_message("SolveBlockEx", worst, "the residual of a column is not finite", R.maxIt);
    return ok ? worst : MGCG_ERROR;
}

// The arguments that every entry point of the loop takes: the handles, the matrix and the vectors of this rank, the partition.
struct CgCall {
    const char* who;                       // the caller's name in its messages
    MgcgComm* comm; MgcgBlas* cublas; MgcgSparse* cusparse;
    Vector* elements; VectorInt* rowOffsets; VectorInt* columnIndeces;
    Vector *x, *b, *Ap, *p, *r;
    int count, nLocal, offset, elementsCount, minJ, maxJ;
};

// One call of the loop: the checks of the arguments, the run's description, the halo plan of p with its overlap schedule, body(R), and the
// plan's release.  handles: the caller's verdict on the handles that only it takes; checks(): its own checks of the arguments, behind the
// common ones.  false: the body did not run (set_error says why).
// A rank whose own arguments are unusable must not simply return: its peers would block in the solve's first collective.  The verdict
// travels in the halo plan's one all-reduce (halo_plan_create, localOk) and every rank leaves.
template <typename Checks, typename Body>
static bool cg_call(const CgCall& c, bool handles, Checks checks, Body body)
{
    bool pre = handles && c.cublas && c.cusparse;
    if (!pre) set_error("%s: null handle", c.who);
    Vector *e = c.elements, *x = c.x, *b = c.b, *Ap = c.Ap, *p = c.p, *r = c.r;
    VectorInt *ro = c.rowOffsets, *ci = c.columnIndeces;
    if (pre && (!e || !ro || !ci || !x || !b || !Ap || !p || !r)) { set_error("%s: null vector handle", c.who); pre = false; }
    if (pre && (c.elementsCount < 0 || c.nLocal < 0 || c.count < c.nLocal)) { set_error("%s: bad sizes", c.who); pre = false; }
    if (pre && (e->size < c.elementsCount || ci->size < c.elementsCount || ro->size < (long long)c.nLocal + 1 || x->size < c.nLocal || b->size < c.nLocal ||
                Ap->size < c.nLocal || r->size < c.nLocal || p->size < c.count)) { set_error("%s: a device vector is smaller than the problem", c.who); pre = false; }
    pre = pre && checks();
    if (pre && (c.offset < 0 || (long long)c.offset + c.nLocal > c.count)) { set_error("%s: bad partition", c.who); pre = false; }
    if (!pre) {
        if (MgcgCommSize(c.comm) > 1 && device_state()) (void)halo_plan_create(c.comm, c.count, c.offset, c.nLocal, c.minJ, c.maxJ, nullptr, 0, true, false);
        return false;
    }
    CgRun R;
    R.ws = &c.cublas->ws; R.cfg = cfg_of(c.cusparse); R.prof = &c.cusparse->prof; R.cusparse = c.cusparse;
    R.comm = c.comm; R.nranks = MgcgCommSize(c.comm); R.multi = comm_multi(c.comm);
    R.elements = e->data; R.rowOffsets = ro->data; R.columnIndeces = ci->data; R.elementsCount = c.elementsCount;
    R.x = x->data; R.b = b->data; R.Ap = Ap->data; R.p = p->data; R.r = r->data; R.pVec = p; R.ApVec = Ap;
    R.count = c.count; R.nLocal = c.nLocal; R.offset = c.offset;
    if (R.multi) {
        R.halo = halo_plan_create(c.comm, c.count, c.offset, c.nLocal, c.minJ, c.maxJ, R.columnIndeces, R.elementsCount, true);
        if (!R.halo) return false;
        if (!cg_plan_overlap(R)) { halo_plan_destroy(R.halo); return false; }
    }
    body(R);
    if (R.halo) halo_plan_destroy(R.halo);
    return true;
}
static bool no_more_checks() { return true; }

// The call of a one-rank export: every row and every column is this rank's.
static CgCall cg_call_one_rank(const char* who, MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elements, VectorInt* rowOffsets, VectorInt* columnIndeces,
                               Vector* x, Vector* b, Vector* Ap, Vector* p, Vector* r, int elementsCount, int count)
{
    return { who, nullptr, cublas, cusparse, elements, rowOffsets, columnIndeces, x, b, Ap, p, r, count, count, 0, elementsCount, 0, count - 1 };
}

static void cg_set_stop(CgRun& R, double allowableResidual, int minIteration, int maxIteration, int rule)
{
    R.tol = allowableResidual; R.minIt = minIteration; R.maxIt = maxIteration; R.rule = rule;
}

// What a variant solver refuses without a device: a null handle (the caller's verdict), k outside 1 .. kMax (noun: what k counts), a stop rule
// that is unknown or, with maxNormWhy (why this loop cannot take it), the max-norm rule, no rows, and k traces beyond what an int can index.
static bool cg_variant_args(const char* who, bool handles, int k, int kMax, const char* noun, int rule, const char* maxNormWhy, int count,
                            const double* residualTrace, int traceCapacity)
{
    if (!handles) set_error("%s: null handle", who);
    else if (k < 1 || k > kMax) set_error("%s: k = %d %s, must be 1 .. %d", who, k, noun, kMax);
    else if (cg_rule_refused(who, rule, maxNormWhy)) return false;
    else if (count < 1) set_error("%s: bad sizes", who);
    else if (residualTrace && traceCapacity > 0 && (long long)k * traceCapacity > 0x7fffffffLL) set_error("%s: trace capacity too large", who);
    else return true;
    return false;
}

// The entry path of the one-column variants' exports (single-reduction CG, MINRES, BiCGStab, preconditioned MINRES, Chebyshev CG), one rank
// and several.  handles: the caller's verdict on the handles that only it takes; checks(): its refusals of its own arguments, which look at
// nothing but those handles; body(R): the solve, whose status is returned.  What is refused where:
//   one rank (no communicator, or one of size 1): there is nobody to agree with, so what needs no device is refused before one is asked for --
//     a null handle first, then checks() -- and then the device;
//   several ranks: nothing is refused in front of cg_call.  A rank with unusable arguments must not simply return: its verdict, checks()
//     included, travels in the halo plan's one all-reduce and every rank leaves with MGCG_ERROR.  The device is asked for only with the
//     handles in hand, which the plan of a refusing rank needs too.
// A rank whose diagonal set-up failed calls with a null dinvVector where the export requires one: that is a null handle, refused by every rank.
// NOT part of the agreement are the values every rank must pass alike -- a shift, a degree and its bounds, whether an optional dinvVector
// is given: the exports say which.  Nothing is enqueued for a call that fails here or in cg_call's checks.
template <typename Checks, typename Body>
static int cg_variant_call(const CgCall& c, bool handles, Checks checks, Body body)
{
    if (MgcgCommSize(c.comm) <= 1) {
        if (!handles) { set_error("%s: null handle", c.who); return MGCG_ERROR; }
        if (!checks()) return MGCG_ERROR;
    }
    if (handles && !device_state()) return MGCG_ERROR;
    int st = MGCG_ERROR;
    cg_call(c, handles, checks, [&](CgRun& R) { st = body(R); });
    return st;
}

// The one-rank exports whose loop keeps its vectors in one work vector (BiCGStab(l), GMRES(m)): what they all take.  jacobi: dinv is a
// handle the export requires; vcycle: the hierarchy is.
struct CgWorkCall {
    const char* who; bool jacobi;
    MgcgBlas* cublas; MgcgSparse* cusparse;
    Vector* elements; VectorInt* rowOffsets; VectorInt* columnIndeces;
    Vector *x, *b, *Ap, *p, *r, *work, *dinv;
    int elementsCount, count;
    double allowableResidual; int minIteration, maxIteration, rule;
    int* iteration; double* residual; double* trueResidual; double* residualTrace; int traceCapacity;
    bool vcycle = false; MgcgMg* mg = nullptr;     // the V-cycle form (SolveGmresMg): the hierarchy is a handle the export requires
};

// The hierarchy of a V-cycle form (SolveMinresMg, SolveBicgstabMg, SolveGmresMg): one rank, `count` rows on level 0 -- whatever matrix it
// was built from.  True: refused.
static bool cg_hierarchy_refused(const char* who, const MgcgMg* mg, int count)
{
    if (mg->nranks != 1 || mg->multi) set_error("%s: the hierarchy was built for %d rank(s)%s; the V-cycle form runs on one rank", who, mg->nranks, mg->multi ? " on the several-ranks path" : "");
    else if (mg->levels < 1 || mg->lv[0].n != count) set_error("%s: the hierarchy has %lld rows on level 0, the matrix has %d", who, mg->levels < 1 ? 0LL : (long long)mg->lv[0].n, count);
    else return false;
    return true;
}

// The loops whose recurrence takes M for one fixed linear map (SolveMgParallel, SolveMinresMg, SolveBicgstabMg, MgcgSolveLobpcgMg): the K-cycle
// is not one (its scalars depend on the vector it is applied to).  True: refused.
static bool cg_kcycle_refused(const char* who, const MgcgMg* mg)
{
    if (mg->cycle == 0) return false;
    set_error("%s: the hierarchy runs the K-cycle (MgSetCycle), which is not a fixed linear map; this loop needs one -- MgSetCycle(mg, 0, 0) restores the V-cycle, SolveMg and SolveGmresMg take the K-cycle", who);
    return true;
}

// Their entry (refusals: cg_variant_call).  params(): the export's refusals of its own sizes, in front of the rule's; slices: how many
// vectors the work vector holds, cg_work_stride(count) apart; noun, value: the size that the short work vector's message names; loop(R): the solve.
template <typename Params, typename Loop>
static int cg_work_vector_call(const CgWorkCall& w, Params params, int slices, const char* noun, int value, Loop loop)
{
    const char* who = w.who;
    const CgCall c = cg_call_one_rank(who, w.cublas, w.cusparse, w.elements, w.rowOffsets, w.columnIndeces, w.x, w.b, w.Ap, w.p, w.r, w.elementsCount, w.count);
    auto checks = [&] {
        if (!params() || cg_rule_refused(who, w.rule, "the loop carries no max|r|")) return false;
        // a count below 1 is the shared checks' to refuse (cg_call, behind these): it asks for no room here, never for a negative amount
        const long long need = slices * cg_work_stride(w.count > 0 ? w.count : 0);
        if (w.work->size < need) {
            set_error("%s: the work vector holds %lld entries, %s = %d needs %lld (%d slices of %lld: the matrix has %d rows)", who, w.work->size, noun, value, need, slices, cg_work_stride(w.count), w.count);
            return false;
        }
        return !(w.jacobi && cg_vector_short(who, "dinv", w.dinv, w.count, "local rows")) && !(w.vcycle && cg_hierarchy_refused(who, w.mg, w.count));
    };
    return cg_variant_call(c, w.cublas && w.cusparse && w.work && (!w.jacobi || w.dinv) && (!w.vcycle || w.mg), checks, [&](CgRun& R) {
        if (R.multi) { set_error("%s: the loop runs on one rank", who); return (int)MGCG_ERROR; }
        if (w.jacobi) R.dinv = cg_dinv_address(R, w.dinv);
        if (w.vcycle) R.mg = w.mg;
        cg_set_stop(R, w.allowableResidual, w.minIteration, w.maxIteration, w.rule);
        cg_note_written({ R.x, R.Ap, R.r, R.p }, w.count);
        cg_note_written({ w.work->data }, slices * cg_work_stride(w.count));
        return loop(R);
    });
}

// BiCGStab(l) (cg_solve_bicgstabl above)
static int bicgstabl_call(const CgWorkCall& w, int ell)
{
    auto params = [&] {
        if (ell >= 1 && ell <= kBicgstablMaxL) return true;
        set_error("%s: ell = %d, must be 1 .. %d", w.who, ell, kBicgstablMaxL);
        return false;
    };
    return cg_work_vector_call(w, params, bicgstabl_slices(ell, w.jacobi), "ell", ell, [&](CgRun& R) {
        return cg_solve_bicgstabl(R, w.who, ell, w.work->data, w.iteration, w.residual, w.trueResidual, w.residualTrace, w.traceCapacity);
    });
}

// GMRES(m) (cg_solve_gmres above); w.vcycle: the flexible form, 2 m + 1 slices
static int gmres_call(const CgWorkCall& w, int m, int orth)
{
    auto params = [&] {
        if (m < 1 || m > kGmresMaxM) set_error("%s: m = %d, must be 1 .. %d", w.who, m, kGmresMaxM);
        else if (orth < 1 || orth > 2) set_error("%s: orth = %d, must be 1 or 2", w.who, orth);
        else return true;
        return false;
    };
    return cg_work_vector_call(w, params, gmres_slices(m, w.jacobi, w.vcycle), "m", m, [&](CgRun& R) {
        return cg_solve_gmres(R, w.who, m, orth, w.work->data, w.iteration, w.residual, w.trueResidual, w.residualTrace, w.traceCapacity);
    });
}

// SolveEx and SolveParallel
static int solve_plain(const CgCall& c, double allowableResidual, int minIteration, int maxIteration, int rule,
                       int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    if (!device_state()) return MGCG_ERROR;
    int st = MGCG_ERROR;
    cg_call(c, true, no_more_checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        st = cg_solve(R, iteration, residual, residualTrace, traceCapacity);
    });
    return st;
}

// The entry of MgcgSolveLobpcg and MgcgSolveLobpcgMg (lob_solve above): what needs no device is refused before one is asked for, and nothing is enqueued for a call that fails.
static int lob_entry(const char* who, bool vcycle, MgcgMg* mg, MgcgBlas* cublas, MgcgSparse* cusparse,
                     Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector, Vector* xVector, Vector* workVector, Vector* dinvVector,
                     int elementsCount, int count, int k, int largest, double allowableResidual, int relative, int minIteration, int maxIteration,
                     int* iteration, double theta[], double residual[], double trueResidual[], int status[], int* restarts, double residualTrace[], int traceCapacity)
{
    if (!cublas || !cusparse || (vcycle && !mg)) { set_error("%s: null handle", who); return MGCG_ERROR; }
    if (!elementsVector || !rowOffsetsVector || !columnIndecesVector || !xVector || !workVector) { set_error("%s: null vector handle", who); return MGCG_ERROR; }
    if (k < 1 || k > kBlockMaxK) { set_error("%s: k = %d eigenpairs, must be 1 .. %d", who, k, kBlockMaxK); return MGCG_ERROR; }
    if (count < 1 || elementsCount < 0) { set_error("%s: bad sizes (count %d, elementsCount %d)", who, count, elementsCount); return MGCG_ERROR; }
    if (3LL * k > count) { set_error("%s: k = %d eigenpairs need a basis of %d columns, the matrix has %d rows", who, k, 3 * k, count); return MGCG_ERROR; }
    if (largest != 0 && largest != 1) { set_error("%s: largest = %d, must be 0 or 1", who, largest); return MGCG_ERROR; }
    if (relative != 0 && relative != 1) { set_error("%s: relative = %d, must be 0 or 1", who, relative); return MGCG_ERROR; }
    if (!(allowableResidual >= 0.0 && allowableResidual <= 1.79e308)) { set_error("%s: allowableResidual is negative or not finite", who); return MGCG_ERROR; }
    if (vcycle && largest) { set_error("%s: largest = 1 is not supported with a hierarchy: its cycle approximates A^-1, which favours the lowest eigenvalues", who); return MGCG_ERROR; }
    if (residualTrace && traceCapacity > 0 && (long long)k * traceCapacity > 0x7fffffffLL) { set_error("%s: trace capacity too large", who); return MGCG_ERROR; }
    if (elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount || rowOffsetsVector->size < (long long)count + 1) {
        set_error("%s: a vector of the matrix is smaller than the matrix (%d stored entries, %d rows)", who, elementsCount, count); return MGCG_ERROR;
    }
    const long long kn = (long long)k * count, need = MgcgLobpcgWorkSize(count, k);
    if (xVector->size < kn) { set_error("%s: the x vector holds %lld entries, k = %d columns of %d rows need %lld", who, xVector->size, k, count, kn); return MGCG_ERROR; }
    // (need > 0 behind the checks of k and count above; were it not, no size would pass for nothing)
    if (need <= 0 || workVector->size < need) { set_error("%s: the work vector holds %lld entries, MgcgLobpcgWorkSize(%d, %d) = %lld", who, workVector->size, count, k, need); return MGCG_ERROR; }
    if (dinvVector && cg_vector_short(who, "dinv", dinvVector, count, "rows")) return MGCG_ERROR;
    if (vcycle && (cg_hierarchy_refused(who, mg, count) || cg_kcycle_refused(who, mg))) return MGCG_ERROR;
    if (!device_state()) return MGCG_ERROR;
    CgRun R;
    R.ws = &cublas->ws; R.cusparse = cusparse; R.nLocal = count; R.count = count;
    cg_set_stop(R, allowableResidual, minIteration, maxIteration, MGCG_RULE_CSHARP);
    if (vcycle && mg->stream != R.ws->stream) { set_error("%s: the hierarchy was set up with another MgcgBlas handle than this call's", who); return MGCG_ERROR; }
    const long long ld = cg_work_stride(count);
    double* w = workVector->data;
    LobRun P{};
    P.ws = R.ws; P.elements = elementsVector->data; P.rowOffsets = rowOffsetsVector->data; P.columnIndeces = columnIndecesVector->data;
    P.n = count; P.ld = ld; P.k = k; P.largest = largest; P.relative = relative; P.pre = vcycle ? 2 : dinvVector ? 1 : 0;
    P.tol = allowableResidual; P.minIt = minIteration; P.maxIt = maxIteration;
    P.X = xVector->data; P.AX = w; P.W = w + k * ld; P.AW = w + 2 * k * ld; P.P = w + 3 * k * ld; P.AP = w + 4 * k * ld; P.Rv = w + 5 * k * ld;
    P.dinv = dinvVector ? dinvVector->data : nullptr;
    cg_note_written({ P.X }, kn);
    cg_note_written({ w }, need);
    return lob_solve(R, P, vcycle ? mg : nullptr, who, iteration, theta, residual, trueResidual, status, restarts, residualTrace, traceCapacity);
}

void preload_solver() { preload_code_object(reinterpret_cast<const void*>(&snapshot_kernel)); }

} // namespace mgcg

using namespace mgcg;

extern "C" {

int SolveEx(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
            Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
            Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
            int elementsCount, int count,
            double allowableResidual, int minIteration, int maxIteration, int rule,
            int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const CgCall c = cg_call_one_rank("SolveEx", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    return solve_plain(c, allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

void Solve(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
           Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
           Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
           int elementsCount, int count,
           double allowableResidual, int minIteration, int maxIteration,
           int* iteration, double* residual)
{
    int it = 0; double res = NAN;
    const int st = SolveEx(cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector,
                           ApVector, pVector, rVector, elementsCount, count, allowableResidual, minIteration, maxIteration,
                           MGCG_RULE_NATIVE, &it, &res, nullptr, 0);
    (void)st;
    if (iteration) *iteration = it + 1;     // the reference returns its post-incremented loop counter (Mgcg.cu:234)
    if (residual) *residual = res;
}

int SolveShifted(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* shiftedPVector,
                 int elementsCount, int count, int k, const double shifts[],
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int iteration[], double residual[], int status[], double residualTrace[], int traceCapacity)
{
    (void)matDescr;
    // what needs no device is refused before one is asked for; nothing is enqueued for a call that fails here or in cg_call's checks
    if (!cg_variant_args("SolveShifted", cublas && cusparse && shiftedPVector, k, kShiftMaxK, "shifts", rule, nullptr, count, residualTrace, traceCapacity)) return MGCG_ERROR;
    if (!shifts) { set_error("SolveShifted: shifts is NULL"); return MGCG_ERROR; }
    for (int j = 0; j < k; ++j)
        if (!(shifts[j] >= 0.0 && shifts[j] <= 1.79e308)) { set_error("SolveShifted: shift %d is %g, must be finite and >= 0", j, shifts[j]); return MGCG_ERROR; }
    if (!device_state()) return MGCG_ERROR;
    const CgCall c = cg_call_one_rank("SolveShifted", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    const long long kn = (long long)k * count;
    auto checks = [&] {
        if (xVector->size < kn || shiftedPVector->size < kn) { set_error("SolveShifted: a device vector is smaller than the problem (x and the direction work space need k * count entries)"); return false; }
        return true;
    };
    int st = MGCG_ERROR;
    cg_call(c, true, checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        analysis_note_write(R.x, sizeof(double) * (size_t)kn);
        analysis_note_write(shiftedPVector->data, sizeof(double) * (size_t)kn);
        st = cg_solve_shifted(R, shiftedPVector->data, k, shifts, iteration, residual, status, residualTrace, traceCapacity);
    });
    return st;
}

int SolveMixed(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* elements32Vector,
               int elementsCount, int count,
               double allowableResidual, int minIteration, int maxIteration, int rule,
               int* iteration, double* residual, int* reliableUpdates, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    // what needs no device is refused before one is asked for; nothing is enqueued for a call that fails here or in cg_call's checks
    if (!cg_variant_args("SolveMixed", cublas && cusparse && elements32Vector, 1, 1, "", rule, "the fp32 recurrence carries no max|r|", count, residualTrace, traceCapacity)) return MGCG_ERROR;
    if (elementsCount < 0) { set_error("SolveMixed: bad sizes"); return MGCG_ERROR; }
    if (elements32Vector->size < ((long long)elementsCount + 1) / 2) {
        set_error("SolveMixed: the elements32 vector holds %lld doubles, the %d floats of MgcgMixedSetup need %lld", elements32Vector->size, elementsCount,
                  ((long long)elementsCount + 1) / 2);
        return MGCG_ERROR;
    }
    if (!device_state()) return MGCG_ERROR;
    const CgCall c = cg_call_one_rank("SolveMixed", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    int st = MGCG_ERROR;
    cg_call(c, true, no_more_checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.r }, count);
        st = cg_solve_mixed(R, (const float*)elements32Vector->data, iteration, residual, reliableUpdates, residualTrace, traceCapacity);
    });
    return st;
}

int SolveBlockEx(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                 int elementsCount, int count, int k,
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int iteration[], double residual[], int status[], double residualTrace[], int traceCapacity)
{
    (void)matDescr;
    if (!device_state()) return MGCG_ERROR;            // (this export asks for the device first)
    if (!cg_variant_args("SolveBlockEx", cublas && cusparse, k, kBlockMaxK, "right-hand sides", rule, nullptr, count, residualTrace, traceCapacity)) return MGCG_ERROR;
    const CgCall c = cg_call_one_rank("SolveBlockEx", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    const long long kn = (long long)k * count;
    auto checks = [&] {
        if (xVector->size < kn || bVector->size < kn || ApVector->size < kn || pVector->size < kn || rVector->size < kn) {
            set_error("SolveBlockEx: a device vector is smaller than the problem (x, b, Ap, p, r need k * count entries)"); return false;
        }
        return true;
    };
    int st = MGCG_ERROR;
    cg_call(c, true, checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        for (double* v : { R.x, R.r, R.p, R.Ap }) analysis_note_write(v, sizeof(double) * (size_t)kn);
        st = cg_solve_block(R, k, iteration, residual, status, residualTrace, traceCapacity);
    });
    return st;
}

int SolveBlockKrylov(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                     Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                     Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                     int elementsCount, int count, int k,
                     double allowableResidual, int minIteration, int maxIteration, int rule,
                     int* iteration, double residual[], int status[], double residualTrace[], int traceCapacity)
{
    (void)matDescr;
    // what needs no device is refused before one is asked for; nothing is enqueued for a call that fails here or in cg_call's checks
    if (!cg_variant_args("SolveBlockKrylov", cublas && cusparse, k, kBlockMaxK, "right-hand sides", rule, "it needs max|r| and the residual block is never formed",
                         count, residualTrace, traceCapacity)) return MGCG_ERROR;
    if (!device_state()) return MGCG_ERROR;
    const CgCall c = cg_call_one_rank("SolveBlockKrylov", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    const long long kn = (long long)k * count;
    auto checks = [&] {
        if (xVector->size < kn || bVector->size < kn || ApVector->size < kn || pVector->size < kn || rVector->size < kn) {
            set_error("SolveBlockKrylov: a device vector is smaller than the problem (x, b, Ap, p, r need k * count entries)"); return false;
        }
        return true;
    };
    int st = MGCG_ERROR;
    cg_call(c, true, checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        for (double* v : { R.x, R.r, R.p, R.Ap }) analysis_note_write(v, sizeof(double) * (size_t)kn);
        st = cg_solve_bkrylov(R, k, iteration, residual, status, residualTrace, traceCapacity);
    });
    return st;
}

int SolveParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                  int count, int countForDevice, int offsetForDevice, int elementsCountForDevice,
                  int minJ, int maxJ,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const CgCall c = { "SolveParallel", comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    return solve_plain(c, allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

double CgSteps(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
               int count, int countForDevice, int offsetForDevice, int elementsCountForDevice,
               int minJ, int maxJ, int steps, int restart)
{
    if (!device_state()) return NAN;
    const CgCall c = { "CgSteps", comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    bool ok = false;
    double res = NAN;
    cg_call(c, true, no_more_checks, [&](CgRun& R) {
        hipStream_t s = R.ws->stream;
        R.rule = MGCG_RULE_NATIVE;
        double* savedTrace = R.ws->trace; const int savedCap = R.ws->traceCap;
        R.ws->trace = nullptr; R.ws->traceCap = 0;
        cg_matrix_setup(R);
        R.haloOnSide = tuning().haloStream.load(std::memory_order_relaxed) != 0;
        if (restart) ok = cg_enqueue_init(R, true);
        else { hipLaunchKernelGGL(clear_done_kernel, dim3(1), dim3(1), 0, s, R.ws->scalars); ok = true; }
        if (ok) cg_xdefer_setup(R, steps);
        const bool report = tuning().verbose.load(std::memory_order_relaxed) >= 2;      // MGCG_VERBOSE=2: is the host or the device the limit?
        const auto h0 = std::chrono::steady_clock::now();
        for (int k = 0; ok && k < steps; ++k) ok = cg_enqueue_iteration(R, false);
        if (ok && R.xDefer > 1) launch_ring_copy_back(s, R.ws->scalars, R.ring, R.nLocal);   // (a non-finite residual stops the loop inside a group)
        if (ok) hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(1), 0, s, R.ws->scalars, R.ws->mirror, (volatile int*)&R.ws->hostScalar[2]);
        const auto h1 = std::chrono::steady_clock::now();
        ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
        if (report && steps > 0) {
            const double enq = std::chrono::duration<double, std::micro>(h1 - h0).count() / steps, all = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count() / steps;
            fprintf(stderr, "[MgcgGpu] CgSteps: host enqueue %.1f us per iteration, enqueue + drain %.1f us per iteration (%d steps)\n", enq, all, steps);
        }
        R.ws->trace = savedTrace; R.ws->traceCap = savedCap;
        res = (double)R.ws->mirror->residual;
    });
    return ok ? res : NAN;
}

int MgcgLastHalo(long long volume[2])
{
    long long v[3]; halo_last(v);
    if (volume) { volume[0] = v[1]; volume[1] = v[2]; }
    return (int)v[0];
}

int MgcgLastVcycleFolds(void) { return t_lastFolds; }

int MgcgLastPlacement(int which, double milliseconds[], int capacity, int* chosen)
{
    if (which < 0 || which > 1) { if (chosen) *chosen = -1; return 0; }
    const int n = t_placementInfo[which][0];
    for (int i = 0; milliseconds && i < n && i < capacity; ++i) milliseconds[i] = t_placementMs[which][i];
    if (chosen) *chosen = t_placementInfo[which][1];
    return n;
}

int MgcgLastOverlapTimes(double microseconds[2])
{
    double t[3]; halo_overlap_last_times(t);
    if (microseconds) { microseconds[0] = t[1]; microseconds[1] = t[2]; }
    return (int)t[0];
}

int MgcgLastOverlap(long long interior[2])
{
    if (interior) { interior[0] = t_lastOverlap[1]; interior[1] = t_lastOverlap[2]; }
    return (int)t_lastOverlap[0];
}

void MgcgProfileSpmv(MgcgSparse* h, int enable)
{
    if (!h) return;
    h->prof.enabled = enable != 0;
    h->prof.used = 0;
}

double MgcgProfileSpmvMs(MgcgSparse* h, int* launches)
{
    if (launches) *launches = 0;
    if (!h) return 0.0;
    std::vector<float> ms((size_t)h->prof.used, 0.0f);
    float longest = 0.0f;
    for (int i = 0; i < h->prof.used; ++i) {
        if (hipEventSynchronize(h->prof.stop[i]) != hipSuccess) continue;
        if (hipEventElapsedTime(&ms[(size_t)i], h->prof.start[i], h->prof.stop[i]) != hipSuccess) ms[(size_t)i] = 0.0f;
        if (ms[(size_t)i] > longest) longest = ms[(size_t)i];
    }
    // launches enqueued after the device raised its stop flag return at their first instruction: not SpMV work
    double total = 0.0;
    for (float t : ms) if (t > 0.05f * longest) { total += t; if (launches) (*launches)++; }
    return total;
}

// ---------------------------------------------------------------- multigrid
MgcgMg* MgSetupParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        int elementsCount, int nx, int ny, int nz, int zBegin, int zEnd,
                        int levels, double omega, int nu, int nuCoarse, double sigma)
{
    DeviceState* d = device_state();
    if (!d) return nullptr;
    const long long nGlobal0 = (long long)nx * ny * nz;
    const int nranks = MgcgCommSize(comm);
    const long long nLocal0 = (long long)nx * ny * (zEnd - zBegin);
    bool pre = true;
    if (!cublas || !cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector) { set_error("MgSetup: null argument"); pre = false; }
    if (pre && (nx < 1 || ny < 1 || nz < 1 || levels < 1 || nu < 1 || nuCoarse < 1 || nGlobal0 > 0x7fffffffLL || zBegin < 0 || zEnd > nz || zBegin >= zEnd)) { set_error("MgSetup: bad parameters"); pre = false; }
    if (pre && (rowOffsetsVector->size < nLocal0 + 1 || elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount)) { set_error("MgSetup: matrix vectors too small"); pre = false; }
    if (pre && nranks > 1 && (nz % nranks != 0 || (zEnd - zBegin) != nz / nranks || zBegin != MgcgCommRank(comm) * (nz / nranks))) {
        set_error("MgSetup: with several ranks the grid must be split into equal z-slabs in rank order"); pre = false;
    }
    if (!comm_agree(comm, pre, "MgSetup")) return nullptr;       // collective: a rank with unusable arguments leaves together with its peers
    hipStream_t s = d->stream;
    MgcgMg* mg = new MgcgMg();
    mg->omega = omega; mg->nu = nu; mg->nuCoarse = nuCoarse; mg->sigma = sigma; mg->stream = s; mg->cfg = cfg_of(cusparse);
    mg->cfg.kernel = 0;   // every level picks its kernel from its own nnz/row
    mg->comm = comm; mg->nranks = nranks; mg->multi = comm_multi(comm);
    mg->haloOnSide = tuning().haloStream.load(std::memory_order_relaxed) != 0;
    const bool multi = mg->multi;
    int* dErr = nullptr;
    int* dmm = nullptr;
    bool ok = MGCG_HIP(hipMalloc((void**)&dErr, sizeof(int))) && MGCG_HIP(hipMemsetAsync(dErr, 0, sizeof(int), s)) && MGCG_HIP(hipMalloc((void**)&dmm, 2 * sizeof(int)));
    // Galerkin matrix of a level from its finer one (two passes: row lengths, then entries).  Whatever it allocated stays in L for MgDestroy.
    auto coarse_matrix = [&](MgLevel& L, const MgLevel& F) -> bool {
        L.ownsMatrix = true;
        int* counts = nullptr;
        bool good = MGCG_HIP(hipMalloc((void**)&L.rowOffsets, sizeof(int) * (size_t)(L.n + 1))) && MGCG_HIP(hipMalloc((void**)&counts, sizeof(int) * (size_t)(L.n > 0 ? L.n : 1)));
        std::vector<int> h((size_t)L.n + 1);
        int err = 0;
        if (good) {
            launch_galerkin(s, F.nx, F.ny, F.nz, F.z0, F.z1, F.elements, F.rowOffsets, F.columnIndeces, sigma, nullptr, counts, nullptr, nullptr, dErr);
            good = MGCG_HIP(hipMemcpyAsync(h.data() + 1, counts, sizeof(int) * (size_t)L.n, hipMemcpyDeviceToHost, s)) &&
                   MGCG_HIP(hipMemcpyAsync(&err, dErr, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        }
        if (counts) (void)hipFree(counts);
        if (!good) return false;
        if (err) { set_error("MgSetup: matrix is not a 27-point-neighbourhood operator on the %dx%dx%d grid", F.nx, F.ny, F.nz); return false; }
        h[0] = 0;
        long long run = 0;
        for (long long i = 1; i <= L.n; ++i) { run += h[(size_t)i]; h[(size_t)i] = (int)run; }   // exclusive scan on the host (set-up only)
        L.nnz = run;
        good = MGCG_HIP(hipMemcpyAsync(L.rowOffsets, h.data(), sizeof(int) * (size_t)(L.n + 1), hipMemcpyHostToDevice, s)) &&
               MGCG_HIP(hipMalloc((void**)&L.elements, sizeof(double) * (size_t)(L.nnz > 0 ? L.nnz : 1))) &&
               MGCG_HIP(hipMalloc((void**)&L.columnIndeces, sizeof(int) * (size_t)(L.nnz > 0 ? L.nnz : 1)));
        if (good) launch_galerkin(s, F.nx, F.ny, F.nz, F.z0, F.z1, F.elements, F.rowOffsets, F.columnIndeces, sigma, L.rowOffsets, nullptr, L.elements, L.columnIndeces, dErr);
        return MGCG_HIP(hipStreamSynchronize(s)) && good;   // (h must outlive the copy)
    };
    bool agreedToLeave = false;
    for (int l = 0; ok && l < levels; ++l) {
        MgLevel L;
        if (l == 0) {
            L.nx = nx; L.ny = ny; L.nz = nz; L.z0 = zBegin; L.z1 = zEnd; L.nnz = elementsCount;
            L.elements = elementsVector->data; L.rowOffsets = rowOffsetsVector->data; L.columnIndeces = columnIndecesVector->data;
        } else {
            const MgLevel& F = mg->lv[l - 1];
            if ((F.nx > 1 && F.nx % 2) || (F.ny > 1 && F.ny % 2) || (F.nz > 1 && F.nz % 2)) break;   // cannot coarsen an odd extent
            if (F.nx == 1 && F.ny == 1 && F.nz == 1) break;
            // the slab must stay aligned: every rank sees the same answer because the slabs are equal
            if (F.nz > 1 && ((F.z0 % 2) || (F.z1 % 2))) break;
            if (nranks > 1 && F.nz == 1) break;
            L.nx = F.nx > 1 ? F.nx / 2 : 1; L.ny = F.ny > 1 ? F.ny / 2 : 1; L.nz = F.nz > 1 ? F.nz / 2 : 1;
            L.z0 = F.nz > 1 ? F.z0 / 2 : 0; L.z1 = F.nz > 1 ? F.z1 / 2 : 1;
        }
        L.nGlobal = (long long)L.nx * L.ny * L.nz;
        L.n = (long long)L.nx * L.ny * (L.z1 - L.z0);
        L.offset = (long long)L.nx * L.ny * L.z0;
        if (l > 0) ok = ok && coarse_matrix(L, mg->lv[l - 1]);
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.dinv, sizeof(double) * (size_t)L.n));
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.xa, sizeof(double) * (size_t)L.nGlobal));
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.r, sizeof(double) * (size_t)L.n));
        if (l > 0 || multi) ok = ok && MGCG_HIP(hipMalloc((void**)&L.xb, sizeof(double) * (size_t)L.nGlobal));
        if (l > 0) ok = ok && MGCG_HIP(hipMalloc((void**)&L.b, sizeof(double) * (size_t)L.n));
        if (ok && multi) {   // halo entries that no neighbour owns (outside the global range) are never read; the rest must start defined
            ok = ok && MGCG_HIP(hipMemsetAsync(L.xa, 0, sizeof(double) * (size_t)L.nGlobal, s)) && MGCG_HIP(hipMemsetAsync(L.xb, 0, sizeof(double) * (size_t)L.nGlobal, s));
        }
        if (ok) launch_extract_dinv(s, L.elements, L.rowOffsets, L.columnIndeces, L.n, L.offset, L.dinv);
        if (ok && L.n > 0) {                              // constant-coefficient operators: one diagonal for all rows
            int differs = 1;
            ok = MGCG_HIP(hipMemsetAsync(dmm, 0, sizeof(int), s));      // (dmm is re-initialised before its min/max use below)
            if (ok) launch_uniform_check(s, L.dinv, L.n, dmm);
            ok = ok && MGCG_HIP(hipMemcpyAsync(&differs, dmm, sizeof(int), hipMemcpyDeviceToHost, s)) &&
                 MGCG_HIP(hipMemcpyAsync(&L.dinvScalar, L.dinv, sizeof(double), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
            L.dinvUniform = ok && differs == 0;
        }
        if (ok) L.dcsr = dcsr_lookup(cusparse, L.elements, L.rowOffsets, L.columnIndeces, L.n, L.nnz, L.offset);
        L.cfg = mg->cfg;
        if (ok && L.nnz >= 8) (void)spmv_period(cusparse, L.rowOffsets, L.columnIndeces, L.n, L.offset, &L.cfg.maxRow);   // longest row of the level (7 on every Galerkin level of a 7-point operator)
        L.cfg.periodRows = (L.nz > 1) ? L.nx * L.ny : 0;       // far band of a 3-D stencil = one grid plane (used only if the caller switched the banded schedule on)
        if (ok && multi) {
            int init[2] = { 0x7fffffff, (int)0x80000000 }, out[2] = { 0, -1 };
            ok = ok && MGCG_HIP(hipMemcpyAsync(dmm, init, sizeof(init), hipMemcpyHostToDevice, s));
            if (ok && L.nnz > 0) launch_minmax_int(s, L.columnIndeces, L.nnz, dmm);
            ok = ok && MGCG_HIP(hipMemcpyAsync(out, dmm, sizeof(out), hipMemcpyDeviceToHost, s));
            ok = ok && MGCG_HIP(hipStreamSynchronize(s));
            L.minJ = out[0]; L.maxJ = out[1];
        }
        if (multi) {
            // the plan and the overlap rule are collective: a rank whose level failed (its slab's matrix is not a stencil operator, an allocation)
            // says so first, and every rank leaves the set-up in the same place
            ok = comm_agree(comm, ok, "MgSetup");
            if (ok) { L.halo = halo_plan_create(comm, L.nGlobal, L.offset, L.n, L.minJ, L.maxJ); ok = comm_agree(comm, L.halo != nullptr, "MgSetup"); }
            agreedToLeave = !ok;                                // (every rank holds the same verdict: no second agreement behind the loop)
            ok = ok && plan_overlap(s, comm, mg->multi, L.rowOffsets, L.columnIndeces, L.n, L.offset, &L.overlap, &L.interior0, &L.interior1, cublas->ws.devInts + 6, L.halo, L.xa, L.nGlobal);
        }
        mg->lv.push_back(L);                                    // (also a level that failed: MgDestroy frees what it had allocated)
        if (!ok) break;
        mg->levels = (int)mg->lv.size();
    }
    ok = ok && MGCG_HIP(hipStreamSynchronize(s));
    if (dErr) (void)hipFree(dErr);
    if (dmm) (void)hipFree(dmm);
    // Deep-halo cycle (mg_deep_level): every level >= 1 gets a full-length right-hand side, the plan that brings `deep` planes of it from
    // the neighbours, and the neighbours' matrix rows for those planes.  Taken when every such level's slab is at least `deep` planes thick
    // (then only the two adjacent ranks are involved); the slabs are equal, so every rank decides the same.  Collective from here on: a
    // local failure is agreed on (comm_agree) before any rank walks into the exchanges.
    bool wantDeep = ok && multi && nu == 1 && mg->levels >= 2 && tuning().deepHalo.load(std::memory_order_relaxed) != 0;
    bool foldsEverywhere = true;
    for (int l = 1; wantDeep && l < mg->levels; ++l) {
        const MgLevel& L = mg->lv[(size_t)l];
        const int d = (l == mg->levels - 1) ? nuCoarse : 2;
        if (L.nz <= 1 || (L.z1 - L.z0) < d || (L.z0 & 1) || ((L.z1 - L.z0) & 1)) wantDeep = false;
    }
    // (a rank that failed outside the agreements above -- before the loop, or in the local tail of a level -- says so here; its peers hear it in
    //  their next agreement, which is this one or the next level's first)
    if (multi && (agreedToLeave || !comm_agree(comm, ok, "MgSetup"))) { MgDestroy(mg); return nullptr; }
    for (int l = 1; ok && wantDeep && l < mg->levels; ++l) {
        MgLevel& L = mg->lv[(size_t)l];
        const long long plane = (long long)L.nx * L.ny;
        const int d = (l == mg->levels - 1) ? nuCoarse : 2;
        L.deep = d;
        L.extZ0 = L.z0 - d < 0 ? 0 : L.z0 - d;
        L.extZ1 = L.z1 + d > L.nz ? L.nz : L.z1 + d;
        L.extBase = (long long)L.extZ0 * plane; L.extRows = (long long)(L.extZ1 - L.extZ0) * plane;
        const long long edge = (long long)d * plane;                                  // rows of d planes
        // my first / last d planes, packed: { rows, nnz, row lengths, values, column ids }
        std::vector<int> ro((size_t)L.n + 1);
        bool lok = MGCG_HIP(hipMemcpyAsync(ro.data(), L.rowOffsets, sizeof(int) * (size_t)(L.n + 1), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        auto pack = [&](long long r0, long long r1, std::vector<double>& out) {
            out.clear();
            if (!lok || r1 <= r0) return;
            const long long k0 = ro[(size_t)r0], k1 = ro[(size_t)r1], K = k1 - k0, Rn = r1 - r0;
            std::vector<double> v((size_t)K); std::vector<int> c((size_t)K);
            lok = lok && (K == 0 || (MGCG_HIP(hipMemcpyAsync(v.data(), L.elements + k0, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, s)) &&
                                     MGCG_HIP(hipMemcpyAsync(c.data(), L.columnIndeces + k0, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost, s)))) && MGCG_HIP(hipStreamSynchronize(s));
            out.reserve((size_t)(2 + Rn + 2 * K));
            out.push_back((double)Rn); out.push_back((double)K);
            for (long long i = r0; i < r1; ++i) out.push_back((double)(ro[(size_t)i + 1] - ro[(size_t)i]));
            out.insert(out.end(), v.begin(), v.end());
            for (int j : c) out.push_back((double)j);
        };
        std::vector<double> toLower, toUpper, fromLower, fromUpper;
        if (L.z0 > 0) pack(0, edge, toLower);                                         // becomes the lower neighbour's upper planes
        if (L.z1 < L.nz) pack(L.n - edge, L.n, toUpper);
        ok = comm_neighbour_exchange_host(comm, toLower, toUpper, fromLower, fromUpper, lok) && lok;
        // the extended slab: [rows from below | my rows | rows from above]
        const long long rowsLo = L.offset - L.extBase, rowsHi = L.extRows - rowsLo - L.n;
        auto header = [&](const std::vector<double>& v, long long rows, long long& K) {
            K = 0;
            if (rows == 0) return v.empty() || nranks == 1;
            if (v.size() < 2 || (long long)v[0] != rows) return false;
            K = (long long)v[1];
            return K >= 0 && (long long)v.size() == 2 + rows + 2 * K;
        };
        long long kLo = 0, kHi = 0;
        if (ok && nranks > 1 && (!header(fromLower, rowsLo, kLo) || !header(fromUpper, rowsHi, kHi))) { set_error("MgSetup: a neighbour sent %zu / %zu values for the halo rows of level %d, not what %lld / %lld rows need", fromLower.size(), fromUpper.size(), l, rowsLo, rowsHi); ok = false; }
        if (ok && nranks == 1 && (rowsLo != 0 || rowsHi != 0)) ok = false;             // (one rank owns every plane: nothing beyond the slab)
        L.extNnz = kLo + L.nnz + kHi;
        if (ok && L.extNnz >= 0x7fffffffLL) { set_error("MgSetup: extended slab of level %d exceeds int32 offsets", l); ok = false; }
        std::vector<int> ero;
        std::vector<int> cLo, cHi;
        if (ok) {
            ero.resize((size_t)L.extRows + 1);
            long long run = 0; size_t at = 0;
            ero[at++] = 0;
            for (long long i = 0; i < rowsLo; ++i) { run += (long long)fromLower[2 + (size_t)i]; ero[at++] = (int)run; }
            for (long long i = 0; i < L.n; ++i) { run += ro[(size_t)i + 1] - ro[(size_t)i]; ero[at++] = (int)run; }
            for (long long i = 0; i < rowsHi; ++i) { run += (long long)fromUpper[2 + (size_t)i]; ero[at++] = (int)run; }
            if (run != L.extNnz) { set_error("MgSetup: halo rows of level %d are inconsistent", l); ok = false; }
            cLo.resize((size_t)kLo); cHi.resize((size_t)kHi);
            for (long long k = 0; k < kLo; ++k) cLo[(size_t)k] = (int)fromLower[2 + (size_t)rowsLo + (size_t)kLo + (size_t)k];
            for (long long k = 0; k < kHi; ++k) cHi[(size_t)k] = (int)fromUpper[2 + (size_t)rowsHi + (size_t)kHi + (size_t)k];
        }
        const size_t nzAlloc = (size_t)(L.extNnz > 0 ? L.extNnz : 1);
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.extElements, sizeof(double) * nzAlloc)) && MGCG_HIP(hipMalloc((void**)&L.extColumnIndeces, sizeof(int) * nzAlloc)) &&
             MGCG_HIP(hipMalloc((void**)&L.extRowOffsets, sizeof(int) * ((size_t)L.extRows + 1))) && MGCG_HIP(hipMalloc((void**)&L.extDinv, sizeof(double) * (size_t)(L.extRows > 0 ? L.extRows : 1))) &&
             MGCG_HIP(hipMalloc((void**)&L.bFull, sizeof(double) * (size_t)L.nGlobal)) && MGCG_HIP(hipMemsetAsync(L.bFull, 0, sizeof(double) * (size_t)L.nGlobal, s));
        if (ok) {
            ok = MGCG_HIP(hipMemcpyAsync(L.extRowOffsets, ero.data(), sizeof(int) * ero.size(), hipMemcpyHostToDevice, s));
            if (kLo > 0) ok = ok && MGCG_HIP(hipMemcpyAsync(L.extElements, fromLower.data() + 2 + rowsLo, sizeof(double) * (size_t)kLo, hipMemcpyHostToDevice, s)) &&
                                    MGCG_HIP(hipMemcpyAsync(L.extColumnIndeces, cLo.data(), sizeof(int) * (size_t)kLo, hipMemcpyHostToDevice, s));
            if (L.nnz > 0) ok = ok && MGCG_HIP(hipMemcpyAsync(L.extElements + kLo, L.elements, sizeof(double) * (size_t)L.nnz, hipMemcpyDeviceToDevice, s)) &&
                                      MGCG_HIP(hipMemcpyAsync(L.extColumnIndeces + kLo, L.columnIndeces, sizeof(int) * (size_t)L.nnz, hipMemcpyDeviceToDevice, s));
            if (kHi > 0) ok = ok && MGCG_HIP(hipMemcpyAsync(L.extElements + kLo + L.nnz, fromUpper.data() + 2 + rowsHi, sizeof(double) * (size_t)kHi, hipMemcpyHostToDevice, s)) &&
                                    MGCG_HIP(hipMemcpyAsync(L.extColumnIndeces + kLo + L.nnz, cHi.data(), sizeof(int) * (size_t)kHi, hipMemcpyHostToDevice, s));
            if (ok && L.extRows > 0) launch_extract_dinv(s, L.extElements, L.extRowOffsets, L.extColumnIndeces, L.extRows, L.extBase, L.extDinv);
            ok = ok && MGCG_HIP(hipStreamSynchronize(s));                               // (the host staging vectors go out of scope)
        }
        if (ok) {                                                                       // the right-hand side moves into the full-length buffer
            if (L.b) (void)hipFree(L.b);
            L.b = L.bFull + L.offset;
        }
        // may the level form its iterates per gather (mg_deep_level)?  One diagonal for every row of the extended slab, power-of-two nx and
        // ny, the row-tile kernel on both matrices.  (A rank-local decision: the results are the same bits either way.)
        if (ok && l < mg->levels - 1) {
            int differs = 1; double d0 = 0.0;
            int* dflag = nullptr;
            bool u = MGCG_HIP(hipMalloc((void**)&dflag, sizeof(int))) && MGCG_HIP(hipMemsetAsync(dflag, 0, sizeof(int), s));
            if (u) launch_uniform_check(s, L.extDinv, L.extRows, dflag);
            u = u && MGCG_HIP(hipMemcpyAsync(&differs, dflag, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipMemcpyAsync(&d0, L.extDinv, sizeof(double), hipMemcpyDeviceToHost, s)) &&
                MGCG_HIP(hipStreamSynchronize(s));
            if (dflag) (void)hipFree(dflag);
            SpmvArgs own{}; own.elements = L.elements; own.columnIndeces = L.columnIndeces; own.elementsCount = (int)L.nnz; own.rowCount = (int)L.n;
            SpmvArgs ext{}; ext.elements = L.extElements; ext.columnIndeces = L.extColumnIndeces; ext.elementsCount = (int)L.extNnz; ext.rowCount = (int)L.extRows;
            const bool can = u && differs == 0 && L.dinvUniform && d0 == L.dinvScalar && L.nx >= 2 && log2_exact(L.nx) >= 1 && log2_exact(L.ny) >= 0 && L.nGlobal < 0x7fffffffLL &&
                             spmv_takes_rowtile(own, L.cfg) && spmv_takes_rowtile(ext, L.cfg);
            foldsEverywhere = foldsEverywhere && can;
        }
        // the plan that brings the `deep` planes of b (collective; every rank reaches it with the same verdict)
        if (!comm_agree(comm, ok, "MgSetup")) { ok = false; break; }
        L.bHalo = halo_plan_create(comm, L.nGlobal, L.offset, L.n, (int)L.extBase, (int)(L.extBase + L.extRows - 1));
        if (!comm_agree(comm, L.bHalo != nullptr, "MgSetup")) { ok = false; break; }
    }
    mg->deep = ok && wantDeep;
    mg->deepFolds = mg->deep && foldsEverywhere;
    if (mg->deep) {       // the loop's residual with room for one grid plane either side (SolveMgParallel keeps r there)
        const MgLevel& L0 = mg->lv[0];
        const size_t len = (size_t)(L0.n + 2LL * L0.nx * L0.ny);
        ok = MGCG_HIP(hipMalloc((void**)&mg->rExt, sizeof(double) * len)) && MGCG_HIP(hipMemsetAsync(mg->rExt, 0, sizeof(double) * len, s)) && MGCG_HIP(hipStreamSynchronize(s));
    }
    // (whether the loop keeps r there decides which exchanges the cycle makes: every rank has the buffer, or the set-up fails on every rank)
    if (multi && wantDeep && !comm_agree(comm, ok, "MgSetup")) ok = false;
    // The finest level of the cycle exchanges its right-hand side and forms x_1 = omega d b per gather -- for the neighbours' columns with the
    // rank's OWN d -- or it exchanges the stored x_1: a decision every rank must take alike, and only when all of them hold the same diagonal.
    if (ok && multi && wantDeep) {
        const MgLevel& L0 = mg->lv[0];
        SpmvArgs probe{}; probe.elements = L0.elements; probe.columnIndeces = L0.columnIndeces; probe.elementsCount = (int)L0.nnz; probe.rowCount = (int)L0.n;
        bool mine = L0.dinvUniform && (L0.dcsr == nullptr || !L0.dcsr->usable) && spmv_takes_rowtile(probe, L0.cfg);
        const std::vector<double> say{ mine ? 1.0 : 0.0, L0.dinvScalar };
        std::vector<double> fromLower, fromUpper;
        ok = comm_neighbour_exchange_host(comm, say, say, fromLower, fromUpper, true);
        for (const std::vector<double>* v : { &fromLower, &fromUpper })
            if (!v->empty()) mine = mine && v->size() == 2 && (*v)[0] == 1.0 && (*v)[1] == L0.dinvScalar;
        bool all = false;
        ok = ok && comm_all(comm, mine, &all);
        mg->deep0 = ok && all;
    }
    if (!ok || mg->levels == 0) { MgDestroy(mg); return nullptr; }
    return mg;
}

MgcgMg* MgSetup(MgcgBlas* cublas, MgcgSparse* cusparse,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                int elementsCount, int nx, int ny, int nz,
                int levels, double omega, int nu, int nuCoarse, double sigma)
{
    return MgSetupParallel(nullptr, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount,
                           nx, ny, nz, 0, nz, levels, omega, nu, nuCoarse, sigma);
}

// ---------------------------------------------------------------- aggregation multigrid: set-up
// The hierarchy of MgSetupParallel with the aggregates taken from the matrix graph (or from the caller) instead of 2x2x2 boxes of a grid; the
// algorithm is written out in include/MgcgGpu.h.  Index bookkeeping -- the scan of a map into aggregate numbers, its counting sort into member
// lists, the scans of row lengths, one flag pair per matching round -- runs on the host, as MgSetupParallel's scan does; every matrix value is
// formed on the device and none travels to the host.
namespace mgcg {

struct AmgDeviceMap { int* agg = nullptr; int* aggOffsets = nullptr; int* members = nullptr; };
static void amg_free(AmgDeviceMap& m)
{
    if (m.agg) (void)hipFree(m.agg);
    if (m.aggOffsets) (void)hipFree(m.aggOffsets);
    if (m.members) (void)hipFree(m.members);
    m = AmgDeviceMap();
}
struct AmgMatrix { double* elements = nullptr; int* rowOffsets = nullptr; int* columnIndeces = nullptr; long long n = 0, nnz = 0; };
static void amg_free(AmgMatrix& m)
{
    if (m.elements) (void)hipFree(m.elements);
    if (m.rowOffsets) (void)hipFree(m.rowOffsets);
    if (m.columnIndeces) (void)hipFree(m.columnIndeces);
    m = AmgMatrix();
}

// out = sigma * P^T A P for the map `map` (row -> aggregate, nc aggregates, none empty) in the contract's order; *dev receives the map and its
// inverted index on the device (the caller frees both results, also after a failure)
static bool amg_galerkin(hipStream_t s, const AmgMatrix& A, const std::vector<int>& map, int nc, double sigma, AmgMatrix* out, AmgDeviceMap* dev)
{
    const size_t n = (size_t)A.n;
    std::vector<int> ro(n + 1), offs((size_t)nc + 1, 0), members(n), expand((size_t)nc + 1, 0);
    if (!MGCG_HIP(hipMemcpyAsync(ro.data(), A.rowOffsets, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, s)) || !MGCG_HIP(hipStreamSynchronize(s))) return false;
    for (size_t i = 0; i < n; ++i) offs[(size_t)map[i] + 1]++;
    for (int I = 0; I < nc; ++I) offs[(size_t)I + 1] += offs[(size_t)I];
    {
        std::vector<int> at(offs.begin(), offs.end() - 1);
        for (size_t i = 0; i < n; ++i) members[(size_t)at[(size_t)map[i]]++] = (int)i;                  // ascending within every aggregate
    }
    long long run = 0;
    for (int I = 0; I < nc; ++I) {
        for (int m = offs[(size_t)I]; m < offs[(size_t)I + 1]; ++m) { const size_t i = (size_t)members[(size_t)m]; run += ro[i + 1] - ro[i]; }
        expand[(size_t)I + 1] = (int)run;
    }
    const size_t scratchLen = (size_t)(run > 0 ? run : 1), ncAlloc = (size_t)(nc > 0 ? nc : 1);
    int *dExpand = nullptr, *scratch = nullptr, *counts = nullptr;
    out->n = nc;
    bool ok = MGCG_HIP(hipMalloc((void**)&dev->agg, sizeof(int) * (n > 0 ? n : 1))) && MGCG_HIP(hipMalloc((void**)&dev->aggOffsets, sizeof(int) * ((size_t)nc + 1))) &&
              MGCG_HIP(hipMalloc((void**)&dev->members, sizeof(int) * (n > 0 ? n : 1))) && MGCG_HIP(hipMalloc((void**)&dExpand, sizeof(int) * ((size_t)nc + 1))) &&
              MGCG_HIP(hipMalloc((void**)&scratch, sizeof(int) * scratchLen)) && MGCG_HIP(hipMalloc((void**)&counts, sizeof(int) * ncAlloc)) &&
              MGCG_HIP(hipMalloc((void**)&out->rowOffsets, sizeof(int) * ((size_t)nc + 1)));
    ok = ok && MGCG_HIP(hipMemcpyAsync(dev->agg, map.data(), sizeof(int) * n, hipMemcpyHostToDevice, s)) &&
         MGCG_HIP(hipMemcpyAsync(dev->aggOffsets, offs.data(), sizeof(int) * ((size_t)nc + 1), hipMemcpyHostToDevice, s)) &&
         MGCG_HIP(hipMemcpyAsync(dev->members, members.data(), sizeof(int) * n, hipMemcpyHostToDevice, s)) &&
         MGCG_HIP(hipMemcpyAsync(dExpand, expand.data(), sizeof(int) * ((size_t)nc + 1), hipMemcpyHostToDevice, s));
    std::vector<int> roC((size_t)nc + 1, 0);
    if (ok) {
        launch_amg_galerkin_count(s, nc, dev->aggOffsets, dev->members, A.rowOffsets, A.columnIndeces, dev->agg, dExpand, scratch, counts);
        ok = MGCG_HIP(hipMemcpyAsync(roC.data() + 1, counts, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    }
    if (ok) {
        long long total = 0;
        for (int I = 1; I <= nc; ++I) { total += roC[(size_t)I]; roC[(size_t)I] = (int)total; }
        out->nnz = total;
        const size_t nzAlloc = (size_t)(total > 0 ? total : 1);
        ok = MGCG_HIP(hipMemcpyAsync(out->rowOffsets, roC.data(), sizeof(int) * ((size_t)nc + 1), hipMemcpyHostToDevice, s)) &&
             MGCG_HIP(hipMalloc((void**)&out->elements, sizeof(double) * nzAlloc)) && MGCG_HIP(hipMalloc((void**)&out->columnIndeces, sizeof(int) * nzAlloc));
        if (ok) launch_amg_galerkin_fill(s, nc, dev->aggOffsets, dev->members, A.elements, A.rowOffsets, A.columnIndeces, dev->agg, dExpand, scratch,
                                         out->rowOffsets, sigma, out->elements, out->columnIndeces);
    }
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;           // (the host staging vectors must outlive the copies)
    if (dExpand) (void)hipFree(dExpand);
    if (scratch) (void)hipFree(scratch);
    if (counts) (void)hipFree(counts);
    return ok;
}

// One matching pass on A: map[i] = the aggregate of row i (pairs and singletons, numbered by their smallest member), *nc = how many
static bool amg_matching_pass(hipStream_t s, const AmgMatrix& A, double theta, std::vector<int>& map, int* nc)
{
    const size_t n = (size_t)A.n, nAlloc = n > 0 ? n : 1;
    double* rowMax = nullptr; int *match = nullptr, *pick = nullptr, *flags = nullptr;
    bool ok = MGCG_HIP(hipMalloc((void**)&rowMax, sizeof(double) * nAlloc)) && MGCG_HIP(hipMalloc((void**)&match, sizeof(int) * nAlloc)) &&
              MGCG_HIP(hipMalloc((void**)&pick, sizeof(int) * nAlloc)) && MGCG_HIP(hipMalloc((void**)&flags, 2 * sizeof(int))) &&
              MGCG_HIP(hipMemsetAsync(match, 0xff, sizeof(int) * nAlloc, s));
    if (ok) launch_amg_row_max(s, A.elements, A.rowOffsets, A.columnIndeces, A.n, rowMax);
    // a round pairs at least the largest remaining edge of a symmetric matrix, so n / 2 rounds is the most there can be; a round in which rows
    // picked and none paired (an unsymmetric matrix: not checked) ends the pass as well
    for (long long round = 0; ok && n > 0 && round <= (long long)n / 2; ++round) {
        int h[2] = { 0, 0 };
        ok = MGCG_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), s));
        if (ok) launch_amg_match_round(s, A.elements, A.rowOffsets, A.columnIndeces, A.n, theta, rowMax, match, pick, flags);
        ok = ok && MGCG_HIP(hipMemcpyAsync(h, flags, 2 * sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        if (!h[0] || !h[1]) break;
    }
    std::vector<int> m(n);
    ok = ok && (n == 0 || (MGCG_HIP(hipMemcpyAsync(m.data(), match, sizeof(int) * n, hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s))));
    if (rowMax) (void)hipFree(rowMax);
    if (match) (void)hipFree(match);
    if (pick) (void)hipFree(pick);
    if (flags) (void)hipFree(flags);
    if (!ok) return false;
    map.assign(n, 0);
    int next = 0;
    for (size_t i = 0; i < n; ++i) {
        const int j = m[i];
        if (j >= 0 && (size_t)j < i) map[i] = map[(size_t)j];     // the smaller member has numbered the pair
        else map[i] = next++;
    }
    *nc = next;
    return true;
}

// The map of one level: `passes` matching passes, pass p > 1 on the unscaled Galerkin matrix of pass p - 1, composed
static bool amg_level_map(hipStream_t s, const AmgMatrix& A, int passes, double theta, std::vector<int>& map, int* nc)
{
    AmgMatrix cur = A, owned;
    bool ok = true;
    for (int p = 1; ok && p <= passes; ++p) {
        std::vector<int> m; int c = 0;
        ok = amg_matching_pass(s, cur, theta, m, &c);
        if (!ok) break;
        if (p == 1) map = m;
        else for (int& v : map) v = m[(size_t)v];
        *nc = c;
        if (c == cur.n || p == passes) break;             // nothing matched: every later pass would see the same graph
        AmgMatrix next; AmgDeviceMap dm;
        ok = amg_galerkin(s, cur, m, c, 1.0, &next, &dm);
        amg_free(dm);
        amg_free(owned);
        owned = next; cur = next;
    }
    amg_free(owned);
    return ok;
}

// What the transposition of a checked matrix leaves on the device: the offsets of A^T and, per entry of A^T, the key (k << 32) | row of A
// (kernels_transpose.hip).  The caller frees it, also after a failure.
struct CsrTransposed { int* offsets = nullptr; unsigned long long* keys = nullptr; };
static void amg_free(CsrTransposed& t)
{
    if (t.offsets) (void)hipFree(t.offsets);
    if (t.keys) (void)hipFree(t.keys);
    t = CsrTransposed();
}

// The offsets of a rows-row matrix start at 0, never descend and end at or below `held`; *nnz = where they end.  Three ints come to the
// host.  false with the message set on a refusal.
static bool csr_check_offsets(const char* who, hipStream_t s, const int* rowOffsets, long long rows, long long held, long long* nnz)
{
    int* dStatus = nullptr;
    int h[3] = { 0x7fffffff, 0, 0 };
    bool ok = MGCG_HIP(hipMalloc((void**)&dStatus, sizeof(h))) && MGCG_HIP(hipMemcpyAsync(dStatus, h, sizeof(h), hipMemcpyHostToDevice, s));
    if (ok) launch_transpose_check_offsets(s, rowOffsets, rows, dStatus);
    ok = ok && MGCG_HIP(hipMemcpyAsync(h, dStatus, sizeof(h), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (dStatus) (void)hipFree(dStatus);
    if (!ok) return false;
    if (h[1] != 0) { set_error("%s: rowOffsets[0] is %d, must be 0", who, h[1]); return false; }
    if (h[0] != 0x7fffffff) { set_error("%s: row %lld: the row offsets descend", who, (long long)h[0]); return false; }
    if (h[2] > held) { set_error("%s: the row offsets end at %lld, the matrix holds %lld entries", who, (long long)h[2], held); return false; }
    *nnz = h[2];
    return true;
}

// The transposition of a matrix whose offsets passed csr_check_offsets and end at nnz: the column check (the flag comes to the host and, on
// a refusal, the one offending row, to name its column; `what` is the word for the bound: "rows" of a square matrix or "columns"), the
// counts, their scan, the claim pass and the sort of every segment.  Complete when it returns.  false with the message set on a refusal.
static bool csr_transpose_device(const char* who, hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long columns, long long nnz,
                                 const char* what, CsrTransposed* out)
{
    const size_t nz = (size_t)nnz, nzAlloc = nz > 0 ? nz : 1, listed = (size_t)std::min<long long>(columns, nnz / (kTransposeShortMax + 1));
    int *cursor = nullptr, *work = nullptr, *dflag = nullptr;
    int bad = 0x7fffffff;
    bool ok = MGCG_HIP(hipMalloc((void**)&out->offsets, sizeof(int) * ((size_t)columns + 1))) && MGCG_HIP(hipMalloc((void**)&dflag, sizeof(int))) &&
              MGCG_HIP(hipMemsetAsync(out->offsets, 0, sizeof(int) * ((size_t)columns + 1), s)) &&
              MGCG_HIP(hipMemcpyAsync(dflag, &bad, sizeof(int), hipMemcpyHostToDevice, s));
    if (ok) launch_transpose_count(s, rowOffsets, columnIndeces, rows, columns, nnz, out->offsets, dflag);
    ok = ok && MGCG_HIP(hipMemcpyAsync(&bad, dflag, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (dflag) (void)hipFree(dflag);
    if (ok && bad != 0x7fffffff) {
        int ends[2] = { 0, 0 };
        ok = MGCG_HIP(hipMemcpy(ends, rowOffsets + bad, sizeof(ends), hipMemcpyDeviceToHost));
        std::vector<int> row((size_t)(ok ? ends[1] - ends[0] : 0));
        ok = ok && MGCG_HIP(hipMemcpy(row.data(), columnIndeces + ends[0], sizeof(int) * row.size(), hipMemcpyDeviceToHost));
        if (!ok) return false;
        for (int c : row)
            if (c < 0 || c >= columns) { set_error("%s: row %lld stores column %d, the matrix has %lld %s", who, (long long)bad, c, columns, what); break; }
        return false;
    }
    ok = ok && exclusive_scan(s, out->offsets, columns + 1);
    ok = ok && MGCG_HIP(hipMalloc((void**)&out->keys, sizeof(unsigned long long) * nzAlloc)) && MGCG_HIP(hipMalloc((void**)&cursor, sizeof(int) * (size_t)columns)) &&
         MGCG_HIP(hipMalloc((void**)&work, sizeof(int) * (listed + 1))) &&
         launch_transpose_claim_and_sort(s, rowOffsets, columnIndeces, rows, columns, nnz, out->offsets, cursor, work, out->keys);
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (cursor) (void)hipFree(cursor);
    if (work) (void)hipFree(work);
    return ok;
}

// *out = S, the symmetric part of A by the contract of MgcgSymmetricPart (include/MgcgGpu.h), in storage of its own (the caller frees it, also
// after a failure).  The merged matrix [A | A^T] -- row i = A's row i in stored order, then the stored entries of column i by source row and
// stored order -- goes through amg_galerkin with the identity map and sigma = 0.5: its contract (entries in stored order, accumulators from
// +0.0, columns ascending, sigma * acc) is S's.  The checks, the transposition (pattern and source list) and the merged matrix are formed on
// the device (kernels_transpose.hip); the flags, the end of the offsets and, on a refusal, one row come to the host.  false with the
// message set on a refusal.
static bool amg_symmetric_part(const char* who, hipStream_t s, const AmgMatrix& A, AmgMatrix* out)
{
    const size_t n = (size_t)A.n;
    long long nnz = 0;
    if (!csr_check_offsets(who, s, A.rowOffsets, A.n, A.nnz, &nnz)) return false;
    if (2 * nnz > 0x7fffffffLL) { set_error("%s: 2 x %lld entries exceed int32 offsets", who, nnz); return false; }
    const size_t mz = 2 * (size_t)nnz, mzAlloc = mz > 0 ? mz : 1;
    CsrTransposed T;
    AmgMatrix M; M.n = A.n; M.nnz = (long long)mz;
    int* dSource = nullptr;
    bool ok = csr_transpose_device(who, s, A.rowOffsets, A.columnIndeces, A.n, A.n, nnz, "rows", &T) &&
              MGCG_HIP(hipMalloc((void**)&M.elements, sizeof(double) * mzAlloc)) && MGCG_HIP(hipMalloc((void**)&M.columnIndeces, sizeof(int) * mzAlloc)) &&
              MGCG_HIP(hipMalloc((void**)&M.rowOffsets, sizeof(int) * (n + 1))) && MGCG_HIP(hipMalloc((void**)&dSource, sizeof(int) * mzAlloc));
    if (ok) {
        launch_transpose_merged(s, A.rowOffsets, A.columnIndeces, T.offsets, T.keys, A.n, nnz, M.rowOffsets, M.columnIndeces, dSource);
        launch_amg_gather_values(s, (long long)mz, dSource, A.elements, M.elements);
        ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipStreamSynchronize(s));
    }
    amg_free(T);                                                                        // (before the product asks for its own storage)
    if (dSource) { (void)hipFree(dSource); dSource = nullptr; }
    if (ok) {
        std::vector<int> identity(n);
        for (size_t i = 0; i < n; ++i) identity[i] = (int)i;
        AmgDeviceMap dm;
        ok = amg_galerkin(s, M, identity, (int)n, 0.5, out, &dm);
        amg_free(dm);
    }
    amg_free(M);
    return ok;
}

// nextMap(l, A_l, map, &nc): 1 = `map` holds level l's aggregates (nc of them), 0 = the hierarchy ends with level l, -1 = error (message set)
typedef std::function<int(int, const AmgMatrix&, std::vector<int>&, int*)> AmgNextMap;
static MgcgMg* amg_setup(const char* who, MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                         int elementsCount, int count, int levels, double omega, int nu, int nuCoarse, double sigma, const AmgNextMap& nextMap)
{
    DeviceState* d = device_state();
    if (!d) return nullptr;
    hipStream_t s = d->stream;
    MgcgMg* mg = new MgcgMg();
    mg->omega = omega; mg->nu = nu; mg->nuCoarse = nuCoarse; mg->sigma = sigma; mg->stream = s; mg->cfg = cfg_of(cusparse);
    mg->cfg.kernel = 0;   // every level picks its kernel from its own nnz/row
    mg->algebraic = true;
    mg->sparse = cusparse;
    int* dflag = nullptr;
    bool ok = MGCG_HIP(hipMalloc((void**)&dflag, sizeof(int)));
    AmgMatrix A; A.elements = elementsVector->data; A.rowOffsets = rowOffsetsVector->data; A.columnIndeces = columnIndecesVector->data; A.n = count; A.nnz = elementsCount;
    for (int l = 0; ok && l < levels; ++l) {
        MgLevel L;
        L.nx = (int)A.n; L.ny = 1; L.nz = 1; L.z0 = 0; L.z1 = 1;
        L.n = A.n; L.nGlobal = A.n; L.offset = 0; L.nnz = A.nnz;
        L.elements = A.elements; L.rowOffsets = A.rowOffsets; L.columnIndeces = A.columnIndeces; L.ownsMatrix = l > 0;
        int bad = 0x7fffffff;
        ok = MGCG_HIP(hipMemcpyAsync(dflag, &bad, sizeof(int), hipMemcpyHostToDevice, s));
        if (ok) launch_amg_check_diagonal(s, L.elements, L.rowOffsets, L.columnIndeces, L.n, dflag);
        ok = ok && MGCG_HIP(hipMemcpyAsync(&bad, dflag, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        if (ok && bad != 0x7fffffff) { set_error("%s: level %d, row %d: the diagonal must be stored, finite and > 0", who, l, bad); ok = false; }
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.dinv, sizeof(double) * (size_t)L.n));
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.xa, sizeof(double) * (size_t)L.n));
        ok = ok && MGCG_HIP(hipMalloc((void**)&L.r, sizeof(double) * (size_t)L.n));
        if (l > 0) ok = ok && MGCG_HIP(hipMalloc((void**)&L.xb, sizeof(double) * (size_t)L.n)) && MGCG_HIP(hipMalloc((void**)&L.b, sizeof(double) * (size_t)L.n));
        if (ok) launch_extract_dinv(s, L.elements, L.rowOffsets, L.columnIndeces, L.n, 0, L.dinv);
        if (ok) {                                         // constant-coefficient operators: one diagonal for all rows (as MgSetupParallel)
            int differs = 1;
            ok = MGCG_HIP(hipMemsetAsync(dflag, 0, sizeof(int), s));
            if (ok) launch_uniform_check(s, L.dinv, L.n, dflag);
            ok = ok && MGCG_HIP(hipMemcpyAsync(&differs, dflag, sizeof(int), hipMemcpyDeviceToHost, s)) &&
                 MGCG_HIP(hipMemcpyAsync(&L.dinvScalar, L.dinv, sizeof(double), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
            L.dinvUniform = ok && differs == 0;
        }
        if (ok) L.dcsr = dcsr_lookup(cusparse, L.elements, L.rowOffsets, L.columnIndeces, L.n, L.nnz, 0);
        L.cfg = mg->cfg;
        if (ok && L.nnz >= 8) (void)spmv_period(cusparse, L.rowOffsets, L.columnIndeces, L.n, 0, &L.cfg.maxRow);
        L.cfg.periodRows = 0;                             // no grid plane: the banded schedule has nothing to go by
        mg->lv.push_back(L);                              // (also a level that failed: MgDestroy frees what it had allocated)
        if (!ok) break;
        mg->levels = (int)mg->lv.size();
        if (l + 1 >= levels) break;
        std::vector<int> map; int nc = 0;
        const int made = nextMap(l, A, map, &nc);
        if (made < 0) { ok = false; break; }
        if (made == 0) break;
        AmgMatrix C; AmgDeviceMap dm;
        ok = amg_galerkin(s, A, map, nc, sigma, &C, &dm);
        MgLevel& F = mg->lv.back();
        F.agg = dm.agg; F.aggOffsets = dm.aggOffsets; F.aggMembers = dm.members;
        if (!ok) { amg_free(C); break; }
        if (C.nnz >= 0x7fffffffLL) { set_error("%s: level %d exceeds int32 offsets", who, l + 1); amg_free(C); ok = false; break; }
        A = C;                                            // the next turn of the loop hands it to its level (which MgDestroy frees, built or not)
    }
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    if (dflag) (void)hipFree(dflag);
    if (!ok || mg->levels == 0) { MgDestroy(mg); return nullptr; }
    return mg;
}

static bool amg_common_arguments(const char* who, MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                                 int elementsCount, int count, int levels, int nu, int nuCoarse)
{
    if (!cublas || !cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector) { set_error("%s: null handle", who); return false; }
    if (levels < 1) { set_error("%s: levels %d, must be >= 1", who, levels); return false; }
    if (count < 1 || elementsCount < 0 || nu < 1 || nuCoarse < 1) { set_error("%s: bad parameters (count %d, elementsCount %d, nu %d, nuCoarse %d)", who, count, elementsCount, nu, nuCoarse); return false; }
    if (rowOffsetsVector->size < (long long)count + 1 || elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount) {
        set_error("%s: matrix vectors too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, (long long)elementsVector->size,
                  (long long)rowOffsetsVector->size, (long long)columnIndecesVector->size, elementsCount, count);
        return false;
    }
    return true;
}

// The colouring of one level for MgSetSmoother(mg, 1) (the algorithm is written out in include/MgcgGpu.h): rounds until every row is
// coloured, one flag per round read by the host as in the matching; then the device check that no row stores an entry of a row of its own
// colour.  The per-colour row lists (ascending) are index bookkeeping and built here on the host.  false with the message set on a refusal.
struct GsColouring { int* rows = nullptr; std::vector<int> offsets, colourOf; };
static bool gs_colour_level(hipStream_t s, const MgLevel& L, int level, GsColouring* out, const char* who = "MgSetSmoother")
{
    const size_t n = (size_t)L.n, nAlloc = n > 0 ? n : 1;
    int *ca = nullptr, *cb = nullptr, *flags = nullptr;       // flags[0]: a row is left; flags[1]: the bad row
    bool ok = MGCG_HIP(hipMalloc((void**)&ca, sizeof(int) * nAlloc)) && MGCG_HIP(hipMalloc((void**)&cb, sizeof(int) * nAlloc)) &&
              MGCG_HIP(hipMalloc((void**)&flags, 2 * sizeof(int))) && MGCG_HIP(hipMemsetAsync(ca, 0xff, sizeof(int) * nAlloc, s));
    bool refused = false;
    // the largest uncoloured row of all is coloured in every round: n rounds at the most
    for (long long round = 0; ok && round < (long long)n; ++round) {
        int h[2] = { 0, 0x7fffffff };
        ok = MGCG_HIP(hipMemcpyAsync(flags, h, sizeof(h), hipMemcpyHostToDevice, s));
        if (ok) launch_gs_colour_round(s, L.rowOffsets, L.columnIndeces, L.n, ca, cb, flags, flags + 1);
        ok = ok && MGCG_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        std::swap(ca, cb);
        if (ok && h[1] != 0x7fffffff) {
            set_error("%s: level %d, row %d: the row's neighbours hold all 64 colours (the multicolour sweep allows 64 per level)", who, level, h[1]);
            refused = true;
            break;
        }
        if (!h[0]) break;
    }
    if (ok && !refused) {
        int bad = 0x7fffffff;
        ok = MGCG_HIP(hipMemcpyAsync(flags + 1, &bad, sizeof(int), hipMemcpyHostToDevice, s));
        if (ok) launch_gs_check(s, L.rowOffsets, L.columnIndeces, L.n, ca, flags + 1);
        ok = ok && MGCG_HIP(hipMemcpyAsync(&bad, flags + 1, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        if (ok && bad != 0x7fffffff) {
            set_error("%s: level %d, row %d: the row stores an entry of a row of its own colour: the pattern is not structurally symmetric "
                      "(some row j stores this row and this row does not store j)", who, level, bad);
            refused = true;
        }
    }
    if (ok && !refused) {
        out->colourOf.assign(n, 0);
        ok = n == 0 || (MGCG_HIP(hipMemcpyAsync(out->colourOf.data(), ca, sizeof(int) * n, hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s)));
    }
    if (ok && !refused) {
        int colours = 0;
        for (size_t i = 0; i < n; ++i) colours = std::max(colours, out->colourOf[i] + 1);
        out->offsets.assign((size_t)colours + 1, 0);
        for (size_t i = 0; i < n; ++i) out->offsets[(size_t)out->colourOf[i] + 1]++;
        for (int c = 0; c < colours; ++c) out->offsets[(size_t)c + 1] += out->offsets[(size_t)c];
        std::vector<int> at(out->offsets.begin(), out->offsets.end() - 1), rows(nAlloc, 0);
        for (size_t i = 0; i < n; ++i) rows[(size_t)at[(size_t)out->colourOf[i]]++] = (int)i;             // ascending within every colour
        ok = MGCG_HIP(hipMalloc((void**)&out->rows, sizeof(int) * nAlloc)) &&
             MGCG_HIP(hipMemcpyAsync(out->rows, rows.data(), sizeof(int) * nAlloc, hipMemcpyHostToDevice, s)) && MGCG_HIP(hipStreamSynchronize(s));
    }
    if (ca) (void)hipFree(ca);
    if (cb) (void)hipFree(cb);
    if (flags) (void)hipFree(flags);
    return ok && !refused;
}

} // namespace mgcg

static MgcgMg* amg_setup_matching(const char* who, MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector,
                                  VectorInt* columnIndecesVector, int elementsCount, int count, int levels, int passes, double theta, int minCoarse,
                                  double omega, int nu, int nuCoarse, double sigma, int strength)
{
    if (!amg_common_arguments(who, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, nu, nuCoarse)) return nullptr;
    if (passes < 1 || passes > 4) { set_error("%s: passes %d, must be 1 .. 4", who, passes); return nullptr; }
    if (!(theta > 0.0 && theta <= 1.0)) { set_error("%s: theta %g, must be in (0, 1]", who, theta); return nullptr; }
    if (strength != 0 && strength != 1) { set_error("%s: strength %d, must be 0 (the matrix's own couplings) or 1 (its symmetric part's)", who, strength); return nullptr; }
    DeviceState* d = device_state();
    if (!d) return nullptr;
    hipStream_t s = d->stream;
    auto nextMap = [&](int, const AmgMatrix& A, std::vector<int>& map, int* nc) -> int {
        if (A.n <= minCoarse) return 0;
        if (strength == 1) {                              // the matching reads S_l = (A_l + A_l^T) / 2; the Galerkin product stays that of A_l
            AmgMatrix S;
            const bool made = amg_symmetric_part(who, s, A, &S) && amg_level_map(s, S, passes, theta, map, nc);
            amg_free(S);
            if (!made) return -1;
        } else if (!amg_level_map(s, A, passes, theta, map, nc)) return -1;
        return (4LL * *nc > 3LL * A.n) ? 0 : 1;           // the next level would keep more than 3/4 of the rows ("nothing matched" included)
    };
    MgcgMg* mg = amg_setup(who, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, omega, nu, nuCoarse, sigma, nextMap);
    if (mg) mg->strength = strength;
    return mg;
}

MgcgMg* MgSetupAggregation(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           int elementsCount, int count, int levels, int passes, double theta, int minCoarse,
                           double omega, int nu, int nuCoarse, double sigma)
{
    return amg_setup_matching("MgSetupAggregation", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, passes, theta,
                              minCoarse, omega, nu, nuCoarse, sigma, 0);
}

MgcgMg* MgSetupAggregationEx(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                             int elementsCount, int count, int levels, int passes, double theta, int minCoarse,
                             double omega, int nu, int nuCoarse, double sigma, int strength)
{
    return amg_setup_matching("MgSetupAggregationEx", cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, passes, theta,
                              minCoarse, omega, nu, nuCoarse, sigma, strength);
}

int MgStrength(const MgcgMg* mg) { return mg ? mg->strength : 0; }

long long MgcgSymmetricPart(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                            int elementsCount, int count, Vector* outElements, VectorInt* outRowOffsets, VectorInt* outColumnIndeces, int outCapacity)
{
    const char* who = "MgcgSymmetricPart";
    if (!cublas || !cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector) { set_error("%s: null handle", who); return -1; }
    const bool countOnly = !outElements && !outRowOffsets && !outColumnIndeces;
    if (!countOnly && (!outElements || !outRowOffsets || !outColumnIndeces)) { set_error("%s: null handle (the three output vectors are given together, or none of them)", who); return -1; }
    if (count < 1 || elementsCount < 0) { set_error("%s: bad parameters (count %d, elementsCount %d)", who, count, elementsCount); return -1; }
    if (2LL * elementsCount > 0x7fffffffLL) { set_error("%s: 2 x elementsCount %d exceeds INT_MAX", who, elementsCount); return -1; }
    if (rowOffsetsVector->size < (long long)count + 1 || elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount) {
        set_error("%s: matrix vectors too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, (long long)elementsVector->size,
                  (long long)rowOffsetsVector->size, (long long)columnIndecesVector->size, elementsCount, count);
        return -1;
    }
    if (!countOnly) {
        if (outCapacity < 0) { set_error("%s: outCapacity %d, must be >= 0", who, outCapacity); return -1; }
        if (outRowOffsets->size < (long long)count + 1 || outElements->size < outCapacity || outColumnIndeces->size < outCapacity) {
            set_error("%s: output vectors too small (%lld values, %lld offsets, %lld columns for a capacity of %d entries in %d rows)", who, (long long)outElements->size,
                      (long long)outRowOffsets->size, (long long)outColumnIndeces->size, outCapacity, count);
            return -1;
        }
    }
    DeviceState* d = device_state();
    if (!d) return -1;
    hipStream_t s = d->stream;
    AmgMatrix A; A.elements = elementsVector->data; A.rowOffsets = rowOffsetsVector->data; A.columnIndeces = columnIndecesVector->data; A.n = count; A.nnz = elementsCount;
    AmgMatrix S;
    bool ok = amg_symmetric_part(who, s, A, &S);
    const long long nnzS = S.nnz;
    if (ok && !countOnly && nnzS > outCapacity) {         // known once the pattern is counted; nothing has been written to the output yet
        set_error("%s: outCapacity %d is below the %lld entries of the symmetric part (2 x elementsCount always suffices)", who, outCapacity, nnzS);
        ok = false;
    }
    if (ok && !countOnly) {
        analysis_note_write(outElements->data, sizeof(double) * (size_t)nnzS);
        analysis_note_write(outColumnIndeces->data, sizeof(int) * (size_t)nnzS);
        analysis_note_write(outRowOffsets->data, sizeof(int) * ((size_t)count + 1));
        ok = MGCG_HIP(hipMemcpyAsync(outRowOffsets->data, S.rowOffsets, sizeof(int) * ((size_t)count + 1), hipMemcpyDeviceToDevice, s)) &&
             (nnzS == 0 || (MGCG_HIP(hipMemcpyAsync(outElements->data, S.elements, sizeof(double) * (size_t)nnzS, hipMemcpyDeviceToDevice, s)) &&
                            MGCG_HIP(hipMemcpyAsync(outColumnIndeces->data, S.columnIndeces, sizeof(int) * (size_t)nnzS, hipMemcpyDeviceToDevice, s))));
        ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    }
    amg_free(S);
    return ok ? nnzS : -1;
}

void MgcgTransposeClassLimits(int* shortMax, int* ldsMax)
{
    if (shortMax) *shortMax = kTransposeShortMax;
    if (ldsMax) *ldsMax = kTransposeLdsMax;
}

long long MgcgCsrTranspose(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           int elementsCount, int rows, int columns, Vector* outElements, VectorInt* outRowOffsets, VectorInt* outColumnIndeces, VectorInt* outSource)
{
    const char* who = "MgcgCsrTranspose";
    if (!cublas || !cusparse || !rowOffsetsVector || !columnIndecesVector || !outRowOffsets || !outColumnIndeces) { set_error("%s: null handle", who); return -1; }
    if ((elementsVector == nullptr) != (outElements == nullptr)) { set_error("%s: null handle (elements and outElements are given together, or neither of them)", who); return -1; }
    if (rows < 1 || columns < 1 || elementsCount < 0) { set_error("%s: bad parameters (rows %d, columns %d, elementsCount %d)", who, rows, columns, elementsCount); return -1; }
    if (rowOffsetsVector->size < (long long)rows + 1 || columnIndecesVector->size < elementsCount || (elementsVector && elementsVector->size < elementsCount)) {
        set_error("%s: matrix vectors too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, elementsVector ? (long long)elementsVector->size : -1LL,
                  (long long)rowOffsetsVector->size, (long long)columnIndecesVector->size, elementsCount, rows);
        return -1;
    }
    if (outRowOffsets->size < (long long)columns + 1 || outColumnIndeces->size < elementsCount || (outElements && outElements->size < elementsCount) ||
        (outSource && outSource->size < elementsCount)) {
        set_error("%s: output vectors too small (%lld values, %lld offsets, %lld columns, %lld sources for %d entries in %d rows of the transpose)", who,
                  outElements ? (long long)outElements->size : -1LL, (long long)outRowOffsets->size, (long long)outColumnIndeces->size,
                  outSource ? (long long)outSource->size : -1LL, elementsCount, columns);
        return -1;
    }
    DeviceState* d = device_state();
    if (!d) return -1;
    hipStream_t s = d->stream;
    long long nnz = 0;
    if (!csr_check_offsets(who, s, rowOffsetsVector->data, rows, elementsCount, &nnz)) return -1;
    CsrTransposed T;
    bool ok = csr_transpose_device(who, s, rowOffsetsVector->data, columnIndecesVector->data, rows, columns, nnz, "columns", &T);
    if (ok) {                                             // every refusal is behind: the outputs are written from here on
        analysis_note_write(outRowOffsets->data, sizeof(int) * ((size_t)columns + 1));
        analysis_note_write(outColumnIndeces->data, sizeof(int) * (size_t)nnz);
        if (outSource) analysis_note_write(outSource->data, sizeof(int) * (size_t)nnz);
        if (outElements) analysis_note_write(outElements->data, sizeof(double) * (size_t)nnz);
        ok = MGCG_HIP(hipMemcpyAsync(outRowOffsets->data, T.offsets, sizeof(int) * ((size_t)columns + 1), hipMemcpyDeviceToDevice, s));
        if (ok) launch_transpose_emit(s, nnz, T.keys, elementsVector ? elementsVector->data : nullptr, outColumnIndeces->data, outSource ? outSource->data : nullptr,
                                      outElements ? outElements->data : nullptr);
        ok = ok && MGCG_HIP(hipGetLastError());
        ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    }
    amg_free(T);
    return ok ? nnz : -1;
}

void MgcgMultiplyClassLimits(int* shortMax, int* ldsMax)
{
    if (shortMax) *shortMax = kMultiplyShortMax;
    if (ldsMax) *ldsMax = kMultiplyLdsMax;
}

// Every stored column of a matrix whose offsets passed csr_check_offsets and end at nnz lies in [0, bound): the flag comes to the host and,
// on a refusal, the one offending row, to name its column (the transposition's message).  false with the message set on a refusal.
static bool csr_check_columns(const char* who, hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long bound, long long nnz)
{
    int* dflag = nullptr;
    int bad = 0x7fffffff;
    bool ok = MGCG_HIP(hipMalloc((void**)&dflag, sizeof(int))) && MGCG_HIP(hipMemcpyAsync(dflag, &bad, sizeof(int), hipMemcpyHostToDevice, s));
    if (ok) launch_multiply_check_columns(s, rowOffsets, columnIndeces, rows, bound, nnz, dflag);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&bad, dflag, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (dflag) (void)hipFree(dflag);
    if (!ok || bad == 0x7fffffff) return ok;
    int ends[2] = { 0, 0 };
    ok = MGCG_HIP(hipMemcpy(ends, rowOffsets + bad, sizeof(ends), hipMemcpyDeviceToHost));
    std::vector<int> row((size_t)(ok ? ends[1] - ends[0] : 0));
    ok = ok && MGCG_HIP(hipMemcpy(row.data(), columnIndeces + ends[0], sizeof(int) * row.size(), hipMemcpyDeviceToHost));
    if (!ok) return false;
    for (int c : row)
        if (c < 0 || c >= bound) { set_error("%s: row %lld stores column %d, the matrix has %lld columns", who, (long long)bad, c, bound); break; }
    return false;
}

long long MgcgCsrMultiply(MgcgBlas* cublas, MgcgSparse* cusparse,
                          Vector* elementsA, VectorInt* rowOffsetsA, VectorInt* columnIndecesA, int elementsCountA,
                          Vector* elementsB, VectorInt* rowOffsetsB, VectorInt* columnIndecesB, int elementsCountB,
                          int rows, int inner, int columns, Vector* outElements, VectorInt* outRowOffsets, VectorInt* outColumnIndeces, int outCapacity)
{
    const char* who = "MgcgCsrMultiply";
    if (!cublas || !cusparse || !rowOffsetsA || !columnIndecesA || !rowOffsetsB || !columnIndecesB) { set_error("%s: null handle", who); return -1; }
    const bool countOnly = !outElements && !outRowOffsets && !outColumnIndeces;
    if ((elementsA == nullptr) != (elementsB == nullptr) || (!countOnly && (elementsA == nullptr) != (outElements == nullptr))) {
        set_error("%s: null handle (elementsA, elementsB and outElements are given together, or none of them)", who);
        return -1;
    }
    if (!countOnly && (!outRowOffsets || !outColumnIndeces)) { set_error("%s: null handle (the output vectors are given together or not at all)", who); return -1; }
    if (rows < 1 || inner < 1 || columns < 1 || elementsCountA < 0 || elementsCountB < 0 || (!countOnly && outCapacity < 0)) {
        set_error("%s: bad parameters (rows %d, inner %d, columns %d, elementsCountA %d, elementsCountB %d, outCapacity %d)", who, rows, inner, columns,
                  elementsCountA, elementsCountB, outCapacity);
        return -1;
    }
    if (rowOffsetsA->size < (long long)rows + 1 || columnIndecesA->size < elementsCountA || (elementsA && elementsA->size < elementsCountA)) {
        set_error("%s: vectors of A too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, elementsA ? (long long)elementsA->size : -1LL,
                  (long long)rowOffsetsA->size, (long long)columnIndecesA->size, elementsCountA, rows);
        return -1;
    }
    if (rowOffsetsB->size < (long long)inner + 1 || columnIndecesB->size < elementsCountB || (elementsB && elementsB->size < elementsCountB)) {
        set_error("%s: vectors of B too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, elementsB ? (long long)elementsB->size : -1LL,
                  (long long)rowOffsetsB->size, (long long)columnIndecesB->size, elementsCountB, inner);
        return -1;
    }
    if (!countOnly && (outRowOffsets->size < (long long)rows + 1 || outColumnIndeces->size < outCapacity || (outElements && outElements->size < outCapacity))) {
        set_error("%s: output vectors too small (%lld values, %lld offsets, %lld columns for a capacity of %d entries in %d rows)", who,
                  outElements ? (long long)outElements->size : -1LL, (long long)outRowOffsets->size, (long long)outColumnIndeces->size, outCapacity, rows);
        return -1;
    }
    DeviceState* d = device_state();
    if (!d) return -1;
    hipStream_t s = d->stream;
    long long nnzA = 0, nnzB = 0;
    if (!csr_check_offsets("MgcgCsrMultiply: A", s, rowOffsetsA->data, rows, elementsCountA, &nnzA) ||
        !csr_check_offsets("MgcgCsrMultiply: B", s, rowOffsetsB->data, inner, elementsCountB, &nnzB) ||
        !csr_check_columns("MgcgCsrMultiply: A", s, rowOffsetsA->data, columnIndecesA->data, rows, inner, nnzA) ||
        !csr_check_columns("MgcgCsrMultiply: B", s, rowOffsetsB->data, columnIndecesB->data, inner, columns, nnzB)) return -1;

    const size_t n = (size_t)rows;
    int *products = nullptr, *work = nullptr, *stat = nullptr, *offsets = nullptr;
    unsigned long long *keys = nullptr, *dTotal = nullptr, total = 0;
    double* scratchProducts = nullptr;
    int hstat[2] = { 0x7fffffff, 0 }, listed = 0;
    // the products of every row, the work list of the rows above the register class
    bool ok = MGCG_HIP(hipMalloc((void**)&products, sizeof(int) * n)) && MGCG_HIP(hipMalloc((void**)&work, sizeof(int) * (n + 1))) &&
              MGCG_HIP(hipMalloc((void**)&stat, sizeof(hstat))) && MGCG_HIP(hipMalloc((void**)&offsets, sizeof(int) * (n + 1))) &&
              MGCG_HIP(hipMalloc((void**)&dTotal, sizeof(total))) &&
              MGCG_HIP(hipMemcpyAsync(stat, hstat, sizeof(hstat), hipMemcpyHostToDevice, s)) && MGCG_HIP(hipMemsetAsync(work, 0, sizeof(int), s)) &&
              MGCG_HIP(hipMemsetAsync(offsets, 0, sizeof(int) * (n + 1), s)) && MGCG_HIP(hipMemsetAsync(dTotal, 0, sizeof(total), s));
    if (ok) launch_multiply_products(s, rowOffsetsA->data, columnIndecesA->data, rowOffsetsB->data, rows, products, work, stat);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(hstat, stat, sizeof(hstat), hipMemcpyDeviceToHost, s)) &&
         MGCG_HIP(hipMemcpyAsync(&listed, work, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (ok && hstat[0] != 0x7fffffff) { set_error("%s: row %lld of the product has more than %d products", who, (long long)hstat[0], 0x7fffffff); ok = false; }
    // the scratch of the global class: one segment of the longest row's products a workgroup, as many workgroups as 1 GiB of keys allows
    const int longest = hstat[1];
    int longGrid = 1;
    MultiplyArgs a = { elementsA ? elementsA->data : nullptr, rowOffsetsA->data, columnIndecesA->data, elementsB ? elementsB->data : nullptr, rowOffsetsB->data,
                       columnIndecesB->data, rows, products, work, offsets, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    if (ok && longest > kMultiplyLdsMax) {
        const long long fit = (1LL << 27) / longest;                                    // 2^27 keys = 1 GiB
        longGrid = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(kMultiplyLongGrid, listed), fit));
        const size_t room = (size_t)longGrid * (size_t)longest;
        ok = MGCG_HIP(hipMalloc((void**)&keys, sizeof(unsigned long long) * room)) && (countOnly || !elementsA || MGCG_HIP(hipMalloc((void**)&scratchProducts, sizeof(double) * room)));
        a.scratchKeys = keys; a.scratchProducts = scratchProducts; a.scratchStride = longest;
    }
    // count: the stored entries of every row of C and, in 64 bits, of C
    ok = ok && launch_multiply_pass(s, a, false, listed, longest, longGrid);
    if (ok) launch_multiply_total(s, offsets, rows, dTotal);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&total, dTotal, sizeof(total), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (ok && total > 0x7fffffffULL) { set_error("%s: the product has %llu entries, more than %d", who, total, 0x7fffffff); ok = false; }
    if (ok && !countOnly && (long long)total > outCapacity) {
        set_error("%s: outCapacity %d is below the %llu entries of the product", who, outCapacity, total);
        ok = false;
    }
    if (ok && !countOnly) {                               // every refusal is behind: the outputs are written from here on
        ok = exclusive_scan(s, offsets, (long long)rows + 1);
        analysis_note_write(outRowOffsets->data, sizeof(int) * (n + 1));
        analysis_note_write(outColumnIndeces->data, sizeof(int) * (size_t)total);
        if (outElements) analysis_note_write(outElements->data, sizeof(double) * (size_t)total);
        a.lengths = nullptr; a.offsetsC = offsets; a.outColumnIndeces = outColumnIndeces->data; a.outElements = outElements ? outElements->data : nullptr;
        ok = ok && MGCG_HIP(hipMemcpyAsync(outRowOffsets->data, offsets, sizeof(int) * (n + 1), hipMemcpyDeviceToDevice, s)) &&
             launch_multiply_pass(s, a, true, listed, longest, longGrid);
    }
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    for (void* p : { (void*)products, (void*)work, (void*)stat, (void*)offsets, (void*)dTotal, (void*)keys, (void*)scratchProducts })
        if (p) (void)hipFree(p);
    return ok ? (long long)total : -1;
}

MgcgMg* MgSetupAggregates(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                          int elementsCount, int count, int levels, const int levelRows[], const int aggregateOf[],
                          double omega, int nu, int nuCoarse, double sigma)
{
    const char* who = "MgSetupAggregates";
    if (!amg_common_arguments(who, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, nu, nuCoarse)) return nullptr;
    if (!levelRows || (levels > 1 && !aggregateOf)) { set_error("%s: null handle", who); return nullptr; }
    if (levelRows[0] != count) { set_error("%s: levelRows[0] is %d, the matrix has %d rows", who, levelRows[0], count); return nullptr; }
    std::vector<long long> first((size_t)levels, 0);      // where level l's map begins in aggregateOf
    for (int l = 0; l + 1 < levels; ++l) {
        const int n = levelRows[l], nc = levelRows[l + 1];
        if (nc < 1 || nc > n) { set_error("%s: levelRows[%d] is %d, must be 1 .. %d", who, l + 1, nc, n); return nullptr; }
        const int* map = aggregateOf + first[(size_t)l];
        std::vector<char> seen((size_t)nc, 0);
        for (int i = 0; i < n; ++i) {
            if (map[i] < 0 || map[i] >= nc) { set_error("%s: level %d, row %d: aggregate id %d out of range (the next level has %d rows)", who, l, i, map[i], nc); return nullptr; }
            seen[(size_t)map[i]] = 1;
        }
        for (int I = 0; I < nc; ++I)
            if (!seen[(size_t)I]) { set_error("%s: level %d: aggregate %d is empty", who, l, I); return nullptr; }
        first[(size_t)l + 1] = first[(size_t)l] + n;
    }
    auto nextMap = [&](int l, const AmgMatrix& A, std::vector<int>& map, int* nc) -> int {
        if (A.n != levelRows[l]) { set_error("%s: level %d has %lld rows, levelRows says %d", who, l, A.n, levelRows[l]); return -1; }
        const int* m = aggregateOf + first[(size_t)l];
        map.assign(m, m + levelRows[l]);
        *nc = levelRows[l + 1];
        return 1;
    };
    return amg_setup(who, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, elementsCount, count, levels, omega, nu, nuCoarse, sigma, nextMap);
}

int MgLevelCopyAggregates(const MgcgMg* mg, int level, int aggregateOf[])
{
    if (!mg || !aggregateOf) { set_error("MgLevelCopyAggregates: null argument"); return -1; }
    if (mg->ilu) { set_error("MgLevelCopyAggregates: the handle is an ILU(0) factor (MgSetupIlu0): it has no aggregates"); return -1; }
    if (!mg->algebraic) { set_error("MgLevelCopyAggregates: a geometric hierarchy has no stored aggregates"); return -1; }
    if (level < 0 || level >= mg->levels - 1 || mg->lv[(size_t)level].agg == nullptr) { set_error("MgLevelCopyAggregates: level %d has no map (the hierarchy has %d levels)", level, mg->levels); return -1; }
    const MgLevel& L = mg->lv[(size_t)level];
    (void)hipStreamSynchronize(mg->stream);
    return MGCG_HIP(hipMemcpy(aggregateOf, L.agg, sizeof(int) * (size_t)L.n, hipMemcpyDeviceToHost)) ? 0 : -1;
}

// The first MgUpdateValues of a hierarchy: the source list of every level that has a map (count, scan, fill: kernels_refresh.hip), the
// shadow buffers and the flags.  One int per level comes to the host: where the offsets end, which must be within the level's entries.
// Whatever a failure leaves allocated stays on the level and is freed by MgDestroy; refreshFlags is set last and says "built".
static bool refresh_build(const char* who, MgcgMg* mg)
{
    hipStream_t s = mg->stream;
    long long bytes = 0;
    bool ok = true;
    for (int l = 0; ok && l < mg->levels; ++l) {
        MgLevel& L = mg->lv[(size_t)l];
        const size_t nAlloc = (size_t)(L.n > 0 ? L.n : 1), nzAlloc = (size_t)(L.nnz > 0 ? L.nnz : 1);
        if (!L.shadowDinv) { ok = MGCG_HIP(hipMalloc((void**)&L.shadowDinv, sizeof(double) * nAlloc)); bytes += (long long)(sizeof(double) * nAlloc); }
        if (ok && l > 0 && !L.shadowElements) { ok = MGCG_HIP(hipMalloc((void**)&L.shadowElements, sizeof(double) * nzAlloc)); bytes += (long long)(sizeof(double) * nzAlloc); }
        if (!ok || l + 1 >= mg->levels || L.agg == nullptr || L.refreshSegments != nullptr) continue;
        const MgLevel& C = mg->lv[(size_t)l + 1];
        const size_t segments = (size_t)C.nnz;
        int* cursor = nullptr;
        int total = 0;
        ok = MGCG_HIP(hipMalloc((void**)&L.refreshSegments, sizeof(int) * (segments + 1))) && MGCG_HIP(hipMalloc((void**)&L.refreshSources, sizeof(int) * nzAlloc)) &&
             MGCG_HIP(hipMalloc((void**)&cursor, sizeof(int) * (segments + 1))) && MGCG_HIP(hipMemsetAsync(L.refreshSegments, 0, sizeof(int) * (segments + 1), s));
        bytes += (long long)(sizeof(int) * (segments + 1) + sizeof(int) * nzAlloc);
        if (ok) launch_refresh_sources_count(s, C.n, L.aggOffsets, L.aggMembers, L.rowOffsets, L.columnIndeces, L.agg, C.rowOffsets, C.columnIndeces, L.refreshSegments);
        ok = ok && MGCG_HIP(hipGetLastError()) && exclusive_scan(s, L.refreshSegments, (long long)segments + 1) &&
             MGCG_HIP(hipMemcpyAsync(cursor, L.refreshSegments, sizeof(int) * (segments + 1), hipMemcpyDeviceToDevice, s)) &&
             MGCG_HIP(hipMemcpyAsync(&total, L.refreshSegments + segments, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        if (ok && (total < 0 || total > L.nnz)) {
            set_error("%s: level %d: the row offsets reach %d entries, the level holds %lld: they are not those of the set-up", who, l, total, L.nnz);
            ok = false;
        }
        if (ok) {
            launch_refresh_sources_fill(s, C.n, L.aggOffsets, L.aggMembers, L.rowOffsets, L.columnIndeces, L.agg, C.rowOffsets, C.columnIndeces, cursor, total, L.refreshSources);
            ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipStreamSynchronize(s));
        }
        if (cursor) (void)hipFree(cursor);
        if (ok) L.refreshCount = total;
        else {                                             // (a list that is not whole must not pass for one at the next call)
            if (L.refreshSegments) (void)hipFree(L.refreshSegments);
            if (L.refreshSources) (void)hipFree(L.refreshSources);
            L.refreshSegments = nullptr; L.refreshSources = nullptr;
        }
    }
    ok = ok && MGCG_HIP(hipMalloc((void**)&mg->refreshScalars, sizeof(double) * (size_t)mg->levels));
    mg->refreshBytes += bytes;
    if (ok) ok = MGCG_HIP(hipMalloc((void**)&mg->refreshFlags, 2 * sizeof(int) * (size_t)mg->levels));
    if (ok) mg->refreshBytes += (long long)((2 * sizeof(int) + sizeof(double)) * (size_t)mg->levels);
    else if (mg->refreshScalars) { (void)hipFree(mg->refreshScalars); mg->refreshScalars = nullptr; }
    return ok;
}

int MgUpdateValues(MgcgMg* mg, Vector* elementsVector, int elementsCount)
{
    const char* who = "MgUpdateValues";
    if (!mg || !elementsVector) { set_error("%s: null argument", who); return -1; }
    if (mg->ilu) { set_error("%s: the handle is an ILU(0) factor: it has no numeric refresh, call MgSetupIlu0 again for the new values", who); return -1; }
    if (!mg->algebraic) {
        set_error("%s: a geometric hierarchy has no numeric refresh, call MgSetup again for the new values (MgSetupAggregates with 2x2x2 box maps builds the same "
                  "hierarchy, which can be refreshed)", who);
        return -1;
    }
    if (mg->nranks != 1 || mg->multi) { set_error("%s: the hierarchy was built for %d rank(s)%s; the refresh runs on one rank", who, mg->nranks, mg->multi ? " on the several-ranks path" : ""); return -1; }
    if (mg->levels < 1 || mg->lv.empty()) { set_error("%s: the hierarchy has no level", who); return -1; }
    if (elementsCount != mg->lv[0].nnz) { set_error("%s: elementsCount %d, the hierarchy was built from %lld entries (MgLevelNnz(mg, 0))", who, elementsCount, mg->lv[0].nnz); return -1; }
    if (elementsVector->size < elementsCount) { set_error("%s: the vector holds %lld values, fewer than the %d entries", who, (long long)elementsVector->size, elementsCount); return -1; }
    if (!device_state()) return -1;
    hipStream_t s = mg->stream;
    const int levels = mg->levels;
    if (mg->refreshFlags == nullptr && !refresh_build(who, mg)) return -1;

    // every level: check, D^-1 and its uniformity on the new values, then the next level's values -- all into the shadow buffers
    std::vector<int> flags(2 * (size_t)levels);
    std::vector<double> scalars((size_t)levels, 0.0);
    for (int l = 0; l < levels; ++l) { flags[2 * (size_t)l] = 0x7fffffff; flags[2 * (size_t)l + 1] = 0; }
    bool ok = MGCG_HIP(hipMemcpyAsync(mg->refreshFlags, flags.data(), sizeof(int) * flags.size(), hipMemcpyHostToDevice, s));
    const double* values = elementsVector->data;
    for (int l = 0; ok && l < levels; ++l) {
        MgLevel& L = mg->lv[(size_t)l];
        launch_amg_check_diagonal(s, values, L.rowOffsets, L.columnIndeces, L.n, mg->refreshFlags + 2 * l);
        launch_extract_dinv(s, values, L.rowOffsets, L.columnIndeces, L.n, 0, L.shadowDinv);
        launch_uniform_check(s, L.shadowDinv, L.n, mg->refreshFlags + 2 * l + 1);
        ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(mg->refreshScalars + l, L.shadowDinv, sizeof(double), hipMemcpyDeviceToDevice, s));
        if (!ok || l + 1 >= levels) break;
        MgLevel& C = mg->lv[(size_t)l + 1];
        analysis_note_write(C.shadowElements, sizeof(double) * (size_t)C.nnz);
        launch_refresh_numeric(s, C.nnz, L.refreshCount, L.refreshSegments, L.refreshSources, values, mg->sigma, C.shadowElements);
        ok = MGCG_HIP(hipGetLastError());
        values = C.shadowElements;
    }
    ok = ok && MGCG_HIP(hipMemcpyAsync(flags.data(), mg->refreshFlags, sizeof(int) * flags.size(), hipMemcpyDeviceToHost, s)) &&
         MGCG_HIP(hipMemcpyAsync(scalars.data(), mg->refreshScalars, sizeof(double) * scalars.size(), hipMemcpyDeviceToHost, s));
    ok = MGCG_HIP(hipStreamSynchronize(s)) && ok;
    MgLevel& L0 = mg->lv[0];
    const bool inPlace = elementsVector->data == L0.elements;
    for (int l = 0; ok && l < levels; ++l)
        if (flags[2 * (size_t)l] != 0x7fffffff) { set_error("%s: level %d, row %d: the diagonal must be stored, finite and > 0", who, l, flags[2 * (size_t)l]); ok = false; }
    if (!ok) {
        // nothing changes hands.  In place, level 0 IS what the caller wrote: its matrix form must not stay that of the values before
        if (inPlace) {
            analysis_note_write(L0.elements, sizeof(double) * (size_t)L0.nnz);
            L0.dcsr = dcsr_lookup(mg->sparse, L0.elements, L0.rowOffsets, L0.columnIndeces, L0.n, L0.nnz, 0);
        }
        return -1;
    }
    analysis_note_write(L0.elements, sizeof(double) * (size_t)L0.nnz);                        // leaves the hierarchy, or was rewritten
    analysis_note_write(elementsVector->data, sizeof(double) * (size_t)L0.nnz);
    L0.elements = elementsVector->data;
    for (int l = 0; l < levels; ++l) {
        MgLevel& L = mg->lv[(size_t)l];
        if (l > 0) {
            analysis_note_write(L.elements, sizeof(double) * (size_t)L.nnz);
            std::swap(L.elements, L.shadowElements);
        }
        std::swap(L.dinv, L.shadowDinv);
        L.dinvUniform = flags[2 * (size_t)l + 1] == 0;
        L.dinvScalar = scalars[(size_t)l];
        L.dcsr = dcsr_lookup(mg->sparse, L.elements, L.rowOffsets, L.columnIndeces, L.n, L.nnz, 0);
    }
    return 0;
}

long long MgUpdateBytes(const MgcgMg* mg) { return mg ? mg->refreshBytes : 0; }

long long MgLevelCopyGalerkinSources(const MgcgMg* mg, int level, int segmentOffsets[], int sources[])
{
    const char* who = "MgLevelCopyGalerkinSources";
    if (!mg) { set_error("%s: null handle", who); return -1; }
    if (mg->ilu || !mg->algebraic) { set_error("%s: the handle is no aggregation hierarchy: it has no Galerkin source lists", who); return -1; }
    if (mg->refreshFlags == nullptr) { set_error("%s: the lists are built by the first MgUpdateValues, which this hierarchy has not seen", who); return -1; }
    if (level < 0 || level >= mg->levels - 1 || mg->lv[(size_t)level].refreshSegments == nullptr) {
        set_error("%s: level %d forms no next level (the hierarchy has %d levels)", who, level, mg->levels);
        return -1;
    }
    const MgLevel& L = mg->lv[(size_t)level];
    const size_t segments = (size_t)mg->lv[(size_t)level + 1].nnz;
    (void)hipStreamSynchronize(mg->stream);
    bool ok = true;
    if (segmentOffsets) ok = ok && MGCG_HIP(hipMemcpy(segmentOffsets, L.refreshSegments, sizeof(int) * (segments + 1), hipMemcpyDeviceToHost));
    if (sources && L.refreshCount > 0) ok = ok && MGCG_HIP(hipMemcpy(sources, L.refreshSources, sizeof(int) * (size_t)L.refreshCount, hipMemcpyDeviceToHost));
    return ok ? L.refreshCount : -1;
}

void MgDestroy(MgcgMg* mg)
{
    if (!mg) return;
    if (mg->stream) (void)hipStreamSynchronize(mg->stream);
    if (mg->rExt) (void)hipFree(mg->rExt);
    if (mg->refreshFlags) (void)hipFree(mg->refreshFlags);
    if (mg->refreshScalars) (void)hipFree(mg->refreshScalars);
    if (mg->ilu) {
        for (void* p : { (void*)mg->ilu->values, (void*)mg->ilu->columns, (void*)mg->ilu->offsets, (void*)mg->ilu->diag, (void*)mg->ilu->pinv, (void*)mg->ilu->rowOf })
            if (p) (void)hipFree(p);
        delete mg->ilu;
    }
    for (auto& L : mg->lv) {
        if (L.ownsMatrix) {       // freed addresses may be handed out again: analyses keyed by them are void
            if (L.elements) { analysis_note_write(L.elements, sizeof(double) * (size_t)(L.nnz > 0 ? L.nnz : 1)); (void)hipFree(L.elements); }
            if (L.rowOffsets) { analysis_note_write(L.rowOffsets, sizeof(int) * (size_t)(L.n + 1)); (void)hipFree(L.rowOffsets); }
            if (L.columnIndeces) { analysis_note_write(L.columnIndeces, sizeof(int) * (size_t)(L.nnz > 0 ? L.nnz : 1)); (void)hipFree(L.columnIndeces); }
        }
        if (L.agg) (void)hipFree(L.agg);
        if (L.aggOffsets) (void)hipFree(L.aggOffsets);
        if (L.aggMembers) (void)hipFree(L.aggMembers);
        if (L.gsRows) (void)hipFree(L.gsRows);
        kcycle_free(L);
        if (L.refreshSegments) (void)hipFree(L.refreshSegments);
        if (L.refreshSources) (void)hipFree(L.refreshSources);
        if (L.shadowElements) { analysis_note_write(L.shadowElements, sizeof(double) * (size_t)(L.nnz > 0 ? L.nnz : 1)); (void)hipFree(L.shadowElements); }
        if (L.shadowDinv) (void)hipFree(L.shadowDinv);
        if (L.dinv) (void)hipFree(L.dinv);
        if (L.xa) (void)hipFree(L.xa);
        if (L.xb) (void)hipFree(L.xb);
        if (L.bFull) { if (L.b == L.bFull + L.offset) L.b = nullptr; (void)hipFree(L.bFull); }      // (b pointed into it -- unless the set-up failed in between)
        if (L.extElements) (void)hipFree(L.extElements);
        if (L.extColumnIndeces) (void)hipFree(L.extColumnIndeces);
        if (L.extRowOffsets) (void)hipFree(L.extRowOffsets);
        if (L.extDinv) (void)hipFree(L.extDinv);
        if (L.bHalo) halo_plan_destroy(L.bHalo);
        if (L.b) (void)hipFree(L.b);
        if (L.r) (void)hipFree(L.r);
        if (L.halo) halo_plan_destroy(L.halo);
        if (L.transferHalo) halo_plan_destroy(L.transferHalo);
    }
    delete mg;
}

int MgSetInterpolation(MgcgMg* mg, int mode)
{
    if (!mg || (mode != 0 && mode != 1)) { set_error("MgSetInterpolation: mode must be 0 (piecewise constant) or 1 (cell-centred linear)"); return -1; }
    if (mg->ilu) { set_error("MgSetInterpolation: the handle is an ILU(0) factor (MgSetupIlu0): it has no transfer operators"); return -1; }
    if (mode == 1 && mg->algebraic) { set_error("MgSetInterpolation: the linear transfer needs a grid; this hierarchy was built from aggregates"); return -1; }
    if (!device_state()) return -1;
    if (mode == 1 && mg->multi) {
        // collective: every rank builds, level by level, the plan that brings one grid plane from each z-neighbour
        for (MgLevel& L : mg->lv) {
            if (L.transferHalo) continue;
            const long long plane = (long long)L.nx * L.ny;
            long long lo = L.offset - plane, hi = L.offset + L.n + plane - 1;
            if (lo < 0) lo = 0;
            if (hi > L.nGlobal - 1) hi = L.nGlobal - 1;
            L.transferHalo = halo_plan_create(mg->comm, L.nGlobal, L.offset, L.n, (int)lo, (int)hi);
            if (!L.transferHalo) return -1;
        }
    }
    mg->interp = mode;
    return 0;
}

int MgSetSmoother(MgcgMg* mg, int mode)
{
    if (!mg) { set_error("MgSetSmoother: null handle"); return -1; }
    if (mode != 0 && mode != 1) { set_error("MgSetSmoother: mode %d, must be 0 (weighted Jacobi) or 1 (multicolour Gauss-Seidel)", mode); return -1; }
    if (mg->ilu) { set_error("MgSetSmoother: the handle is an ILU(0) factor (MgSetupIlu0): it has no smoother"); return -1; }
    if (mode == 1 && !mg->algebraic) {
        set_error("MgSetSmoother: the Gauss-Seidel smoother needs every level stored; this hierarchy was built from a grid (MgSetupAggregates with 2x2x2 box maps builds the same hierarchy)");
        return -1;
    }
    if (mode == 1 && mg->nuCoarse % 2 != 0) {
        set_error("MgSetSmoother: nuCoarse %d, must be even: the last level alternates forward and backward sweeps and an odd count is not a symmetric operator", mg->nuCoarse);
        return -1;
    }
    if (!device_state()) return -1;
    if (mg->stream) (void)hipStreamSynchronize(mg->stream);          // no cycle in flight reads the lists that go
    std::vector<GsColouring> made;
    if (mode == 1) {
        made.resize((size_t)mg->levels);
        for (int l = 0; l < mg->levels; ++l) {
            if (gs_colour_level(mg->stream, mg->lv[(size_t)l], l, &made[(size_t)l])) continue;
            for (GsColouring& g : made) if (g.rows) (void)hipFree(g.rows);      // refused: the hierarchy stays as it was
            return -1;
        }
    }
    for (int l = 0; l < mg->levels; ++l) {
        MgLevel& L = mg->lv[(size_t)l];
        if (L.gsRows) (void)hipFree(L.gsRows);
        L.gsRows = nullptr; L.gsOffsets.clear(); L.gsColourOf.clear();
        if (mode == 1) { L.gsRows = made[(size_t)l].rows; L.gsOffsets.swap(made[(size_t)l].offsets); L.gsColourOf.swap(made[(size_t)l].colourOf); }
    }
    mg->smoother = mode;
    return 0;
}

int MgSmoother(const MgcgMg* mg) { return mg ? mg->smoother : 0; }

// The K-cycle (the contract is written out in include/MgcgGpu.h; kernels_kcycle.hip).  Mode 1 allocates the K step's vectors on every level
// that has a finer level and a map of its own; mode 0 frees them.  Nothing else of the hierarchy changes.
int MgSetCycle(MgcgMg* mg, int cycle, int inner)
{
    if (!mg) { set_error("MgSetCycle: null handle"); return -1; }
    if (cycle != 0 && cycle != 1) { set_error("MgSetCycle: cycle %d, must be 0 (V-cycle) or 1 (K-cycle)", cycle); return -1; }
    if (inner != 0 && inner != 1) { set_error("MgSetCycle: inner %d, must be 0 (conjugate steps) or 1 (minimal-residual steps)", inner); return -1; }
    if (mg->ilu) { set_error("MgSetCycle: the handle is an ILU(0) factor (MgSetupIlu0): it has no cycle"); return -1; }
    if (!mg->algebraic) {
        set_error("MgSetCycle: the K-cycle needs every level stored; this hierarchy was built from a grid (MgSetupAggregates with 2x2x2 box maps builds the same hierarchy)");
        return -1;
    }
    if (mg->nranks != 1 || mg->multi) { set_error("MgSetCycle: the hierarchy was built for %d rank(s)%s; the K-cycle runs on one rank", mg->nranks, mg->multi ? " on the several-ranks path" : ""); return -1; }
    if (!device_state()) return -1;
    if (mg->stream) (void)hipStreamSynchronize(mg->stream);          // no cycle in flight reads the vectors that go
    if (cycle == 1 && mg->cycle == 0) {
        bool ok = true;
        for (int l = 1; ok && l + 1 < mg->levels; ++l) {
            MgLevel& L = mg->lv[(size_t)l];
            const size_t bytes = sizeof(double) * (size_t)(L.n > 0 ? L.n : 1);
            for (double** p : { &L.kSpare, &L.kv1, &L.kv2, &L.krr }) ok = ok && MGCG_HIP(hipMalloc((void**)p, bytes));
            ok = ok && MGCG_HIP(hipMalloc((void**)&L.kPartials, sizeof(double) * (size_t)kKcycleSums * kMaxGrid));
        }
        if (!ok) {                                                   // refused: the hierarchy stays in V mode
            for (MgLevel& L : mg->lv) kcycle_free(L);
            return -1;
        }
    }
    if (cycle == 0) for (MgLevel& L : mg->lv) kcycle_free(L);
    mg->cycle = cycle; mg->cycleInner = cycle == 1 ? inner : 0;
    return 0;
}

int MgCycle(const MgcgMg* mg) { return mg ? mg->cycle : 0; }
int MgCycleInner(const MgcgMg* mg) { return mg ? mg->cycleInner : 0; }

int MgLevelColours(const MgcgMg* mg, int level)
{
    if (!mg || level < 0 || level >= mg->levels) { set_error("MgLevelColours: bad level"); return -1; }
    return mg->smoother == 1 ? (int)mg->lv[(size_t)level].gsOffsets.size() - 1 : 0;
}

int MgLevelCopyColours(const MgcgMg* mg, int level, int colourOf[])
{
    if (!mg || !colourOf) { set_error("MgLevelCopyColours: null argument"); return -1; }
    if (level < 0 || level >= mg->levels) { set_error("MgLevelCopyColours: level %d, the hierarchy has %d levels", level, mg->levels); return -1; }
    if (mg->ilu) { set_error("MgLevelCopyColours: the handle is an ILU(0) factor (MgSetupIlu0): MgIluCopyFactor hands out its order (rowOf)"); return -1; }
    if (mg->smoother != 1) { set_error("MgLevelCopyColours: the hierarchy smooths with weighted Jacobi: it has no colours (MgSetSmoother(mg, 1))"); return -1; }
    const MgLevel& L = mg->lv[(size_t)level];
    std::copy(L.gsColourOf.begin(), L.gsColourOf.end(), colourOf);
    return 0;
}

// Multicolour ILU(0) (the contract is written out in include/MgcgGpu.h; kernels_ilu.hip).  What comes to the host: the flags, the colour
// of every row (gs_colour_level) and -- on a refused pivot -- one int and one double; what goes to the device from it: the two permutations.
MgcgMg* MgSetupIlu0(MgcgBlas* cublas, MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    int elementsCount, int count, double shift)
{
    const char* who = "MgSetupIlu0";
    if (!cublas || !cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector) { set_error("%s: null handle", who); return nullptr; }
    if (count < 1 || elementsCount < 0) { set_error("%s: bad parameters (count %d, elementsCount %d)", who, count, elementsCount); return nullptr; }
    if (rowOffsetsVector->size < (long long)count + 1 || elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount) {
        set_error("%s: matrix vectors too small (%lld values, %lld offsets, %lld columns for %d entries in %d rows)", who, (long long)elementsVector->size,
                  (long long)rowOffsetsVector->size, (long long)columnIndecesVector->size, elementsCount, count);
        return nullptr;
    }
    if (!(shift >= 0.0) || !(shift <= 1.7976931348623157e308)) { set_error("%s: shift %g, must be finite and >= 0", who, shift); return nullptr; }
    DeviceState* d = device_state();
    if (!d) return nullptr;
    hipStream_t s = d->stream;
    const double* elements = elementsVector->data;
    const int *rowOffsets = rowOffsetsVector->data, *columnIndeces = columnIndecesVector->data;
    const size_t n = (size_t)count;
    const int kNone = 0x7fffffff;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    long long nnz = 0;
    if (!csr_check_offsets(who, s, rowOffsets, count, elementsCount, &nnz)) return nullptr;

    MgcgMg* mg = new MgcgMg();
    MgIlu* F = mg->ilu = new MgIlu();                     // from here on MgDestroy frees whatever a failed set-up had allocated
    mg->omega = 1.0; mg->stream = s; mg->cfg = cfg_of(cusparse); mg->algebraic = true;
    MgLevel L;
    L.nx = count; L.ny = 1; L.nz = 1; L.z0 = 0; L.z1 = 1;
    L.n = count; L.nGlobal = count; L.offset = 0; L.nnz = nnz;
    L.elements = const_cast<double*>(elements); L.rowOffsets = const_cast<int*>(rowOffsets); L.columnIndeces = const_cast<int*>(columnIndeces); L.ownsMatrix = false;
    L.cfg = mg->cfg;
    F->nnz = nnz;
    F->lanes = (double)nnz <= 4.0 * (double)count ? 4 : ((double)nnz <= 10.0 * (double)count ? 8 : 16);
    const size_t nzAlloc = nnz > 0 ? (size_t)nnz : 1;

    int *dflags = nullptr, *dNewOf = nullptr;
    double* dPartials = nullptr;
    int h[3] = { kNone, kNone, kNone };
    bool ok = MGCG_HIP(hipMalloc((void**)&dflags, sizeof(h))) && MGCG_HIP(hipMemcpyAsync(dflags, h, sizeof(h), hipMemcpyHostToDevice, s));
    if (ok) launch_ilu_check_rows(s, rowOffsets, columnIndeces, count, dflags);
    ok = ok && MGCG_HIP(hipMemcpyAsync(h, dflags, sizeof(h), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (ok && h[0] != kNone) { set_error("%s: row %d stores a column outside [0, %d)", who, h[0], count); ok = false; }
    else if (ok && h[1] != kNone) { set_error("%s: row %d is empty", who, h[1]); ok = false; }
    else if (ok && h[2] != kNone) { set_error("%s: row %d stores no diagonal entry", who, h[2]); ok = false; }

    // the colours and the order: new row = position in the list sorted by (colour, row)
    GsColouring colouring;
    std::vector<int> newOf;
    ok = ok && gs_colour_level(s, L, 0, &colouring, who);
    F->rowOf = colouring.rows;
    const auto t1 = now();
    if (ok) {
        F->colourOffsets = colouring.offsets;
        std::vector<int> at(colouring.offsets.begin(), colouring.offsets.end() - 1);
        newOf.resize(n);
        for (size_t i = 0; i < n; ++i) newOf[i] = at[(size_t)colouring.colourOf[i]]++;
        ok = MGCG_HIP(hipMalloc((void**)&dNewOf, sizeof(int) * n)) && MGCG_HIP(hipMemcpyAsync(dNewOf, newOf.data(), sizeof(int) * n, hipMemcpyHostToDevice, s)) &&
             MGCG_HIP(hipStreamSynchronize(s));
    }
    // B, every row sorted by new column
    ok = ok && MGCG_HIP(hipMalloc((void**)&F->offsets, sizeof(int) * (n + 1))) && MGCG_HIP(hipMalloc((void**)&F->values, sizeof(double) * nzAlloc)) &&
         MGCG_HIP(hipMalloc((void**)&F->columns, sizeof(int) * nzAlloc)) && MGCG_HIP(hipMalloc((void**)&F->diag, sizeof(int) * n)) &&
         MGCG_HIP(hipMalloc((void**)&F->pinv, sizeof(double) * n)) && MGCG_HIP(hipMalloc((void**)&L.xa, sizeof(double) * n)) &&
         MGCG_HIP(hipMalloc((void**)&L.xb, sizeof(double) * n)) && MGCG_HIP(hipMalloc((void**)&dPartials, sizeof(double) * 2 * (size_t)kMaxGrid));
    if (ok) launch_ilu_lengths(s, rowOffsets, F->rowOf, count, F->offsets);
    ok = ok && MGCG_HIP(hipGetLastError()) && exclusive_scan(s, F->offsets, (long long)count + 1);
    int bad = kNone;
    ok = ok && MGCG_HIP(hipMemcpyAsync(dflags, &bad, sizeof(int), hipMemcpyHostToDevice, s));
    if (ok) launch_ilu_build(s, elements, rowOffsets, columnIndeces, F->rowOf, dNewOf, count, shift, F->offsets, F->values, F->columns, F->diag, dflags, F->lanes);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&bad, dflags, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
    if (ok && bad != kNone) { set_error("%s: row %d stores a column twice", who, bad); ok = false; }
    const auto t2 = now();
    // the factor: one launch per colour, the pivot flag read after each
    const int colours = ok ? (int)F->colourOffsets.size() - 1 : 0;
    for (int c = 0; ok && c < colours; ++c) {
        launch_ilu_factor(s, F->colourOffsets[(size_t)c], F->colourOffsets[(size_t)c + 1] - F->colourOffsets[(size_t)c], F->offsets, F->columns, F->diag, F->values,
                          F->pinv, F->rowOf, dflags, F->lanes);
        ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&bad, dflags, sizeof(int), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));
        if (ok && bad != kNone) {
            int where = 0;
            double pivot = 0.0;
            if (MGCG_HIP(hipMemcpy(&where, F->diag + newOf[(size_t)bad], sizeof(int), hipMemcpyDeviceToHost)) && MGCG_HIP(hipMemcpy(&pivot, F->values + where, sizeof(double), hipMemcpyDeviceToHost)))
                set_error("%s: row %d: the pivot is %g, zero or not finite: this matrix has no ILU(0) factor in the colour order (shift > 0 factors A + shift * diag(A))", who, bad, pivot);
            ok = false;
        }
    }
    if (ok) {
        const int blocks = launch_ilu_pivot_range(s, F->values, F->diag, count, dPartials);
        std::vector<double> partials(2 * (size_t)blocks);
        ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(partials.data(), dPartials, sizeof(double) * partials.size(), hipMemcpyDeviceToHost, s)) &&
             MGCG_HIP(hipStreamSynchronize(s));
        F->pivotMin = partials[0]; F->pivotMax = partials[1];
        for (int b = 1; ok && b < blocks; ++b) { F->pivotMin = std::min(F->pivotMin, partials[2 * (size_t)b]); F->pivotMax = std::max(F->pivotMax, partials[2 * (size_t)b + 1]); }
    }
    const auto t3 = now();
    F->setupMs[0] = ms(t0, t1); F->setupMs[1] = ms(t1, t2); F->setupMs[2] = ms(t2, t3);
    if (dflags) (void)hipFree(dflags);
    if (dNewOf) (void)hipFree(dNewOf);
    if (dPartials) (void)hipFree(dPartials);
    mg->lv.push_back(L);                                  // (also after a failure: MgDestroy frees what it had allocated)
    mg->levels = 1;
    if (!ok) { MgDestroy(mg); return nullptr; }
    return mg;
}

int MgIsIlu(const MgcgMg* mg) { return (mg && mg->ilu) ? 1 : 0; }

int MgIluColours(const MgcgMg* mg)
{
    if (!mg || !mg->ilu) { set_error("MgIluColours: the handle is not an ILU(0) factor (MgSetupIlu0)"); return -1; }
    return (int)mg->ilu->colourOffsets.size() - 1;
}

int MgIluPivotRange(const MgcgMg* mg, double* smallest, double* largest)
{
    if (!mg || !mg->ilu) { set_error("MgIluPivotRange: the handle is not an ILU(0) factor (MgSetupIlu0)"); return -1; }
    if (smallest) *smallest = mg->ilu->pivotMin;
    if (largest) *largest = mg->ilu->pivotMax;
    return 0;
}

int MgIluSetupMs(const MgcgMg* mg, double ms[3])
{
    if (!mg || !mg->ilu || !ms) { set_error("MgIluSetupMs: the handle is not an ILU(0) factor (MgSetupIlu0), or a null argument"); return -1; }
    std::copy(mg->ilu->setupMs, mg->ilu->setupMs + 3, ms);
    return 0;
}

long long MgIluCopyFactor(const MgcgMg* mg, double elements[], int columnIndeces[], int rowOffsets[], int diagonal[], int rowOf[])
{
    if (!mg || !mg->ilu) { set_error("MgIluCopyFactor: the handle is not an ILU(0) factor (MgSetupIlu0)"); return -1; }
    const MgIlu& F = *mg->ilu;
    const size_t n = (size_t)mg->lv[0].n, nz = (size_t)F.nnz;
    if (elements || columnIndeces || rowOffsets || diagonal || rowOf) (void)hipStreamSynchronize(mg->stream);
    bool ok = true;
    if (elements) ok = ok && MGCG_HIP(hipMemcpy(elements, F.values, sizeof(double) * nz, hipMemcpyDeviceToHost));
    if (columnIndeces) ok = ok && MGCG_HIP(hipMemcpy(columnIndeces, F.columns, sizeof(int) * nz, hipMemcpyDeviceToHost));
    if (rowOffsets) ok = ok && MGCG_HIP(hipMemcpy(rowOffsets, F.offsets, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    if (diagonal) ok = ok && MGCG_HIP(hipMemcpy(diagonal, F.diag, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (rowOf) ok = ok && MGCG_HIP(hipMemcpy(rowOf, F.rowOf, sizeof(int) * n, hipMemcpyDeviceToHost));
    return ok ? F.nnz : -1;
}

int MgLevels(const MgcgMg* mg) { return mg ? mg->levels : 0; }
long long MgLevelRows(const MgcgMg* mg, int l) { return (mg && l >= 0 && l < mg->levels) ? mg->lv[l].n : -1; }
long long MgLevelNnz(const MgcgMg* mg, int l) { return (mg && l >= 0 && l < mg->levels) ? mg->lv[l].nnz : -1; }

void MgLevelCopyCsr(const MgcgMg* mg, int l, double elements[], int columnIndeces[], int rowOffsets[])
{
    if (!mg || l < 0 || l >= mg->levels) { set_error("MgLevelCopyCsr: bad level"); return; }
    const MgLevel& L = mg->lv[l];
    (void)hipStreamSynchronize(mg->stream);
    (void)MGCG_HIP(hipMemcpy(elements, L.elements, sizeof(double) * (size_t)L.nnz, hipMemcpyDeviceToHost));
    (void)MGCG_HIP(hipMemcpy(columnIndeces, L.columnIndeces, sizeof(int) * (size_t)L.nnz, hipMemcpyDeviceToHost));
    (void)MGCG_HIP(hipMemcpy(rowOffsets, L.rowOffsets, sizeof(int) * (size_t)(L.n + 1), hipMemcpyDeviceToHost));
}
void MgLevelCopyDinv(const MgcgMg* mg, int l, double dinv[])
{
    if (!mg || l < 0 || l >= mg->levels) { set_error("MgLevelCopyDinv: bad level"); return; }
    if (mg->ilu) { set_error("MgLevelCopyDinv: the handle is an ILU(0) factor (MgSetupIlu0): it keeps no D^-1 (MgIluCopyFactor hands out the factor)"); return; }
    (void)hipStreamSynchronize(mg->stream);
    (void)MGCG_HIP(hipMemcpy(dinv, mg->lv[l].dinv, sizeof(double) * (size_t)mg->lv[l].n, hipMemcpyDeviceToHost));
}

void MgApply(MgcgMg* mg, const double* r, double* z)
{
    if (!device_state()) return;
    if (!mg || !r || !z) { set_error("MgApply: null argument"); return; }
    (void)mg_apply(mg, r, z, nullptr);
    (void)MGCG_HIP(hipGetLastError());
}

int SolveMgParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* zVector,
                    int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                    double allowableResidual, int minIteration, int maxIteration, int rule,
                    int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    if (!device_state()) return MGCG_ERROR;
    const CgCall c = { "SolveMg", comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        if (zVector->size < countForDevice || mg->lv[0].n != countForDevice || mg->lv[0].nGlobal != count || mg->lv[0].offset != offsetForDevice) {
            set_error("SolveMg: z vector or hierarchy does not match the problem"); return false;
        }
        if (mg->nranks != MgcgCommSize(comm) || mg->multi != comm_multi(comm)) { set_error("SolveMg: the hierarchy was built for %d rank(s)%s", mg->nranks, mg->multi ? " on the several-ranks path" : ""); return false; }
        if (rule == MGCG_RULE_HANDMADECL || rule == MGCG_RULE_VIENNACL) { set_error("SolveMg supports the 2-norm absolute rules only"); return false; }
        if (comm != nullptr && cg_kcycle_refused("SolveMgParallel", mg)) return false;     // (SolveMg, one rank without a communicator, takes the K-cycle)
        return true;
    };
    int st = MGCG_ERROR;
    cg_call(c, mg && zVector, checks, [&](CgRun& R) {
        R.mg = mg; R.z = zVector->data;
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        // deep-halo cycle: the loop keeps r in the hierarchy's extended buffer (room for the halo planes the cycle's one exchange brings) and the
        // caller's vector receives it when the solve is over
        const bool rExtended = R.multi && mg->deep && mg->rExt != nullptr;
        if (rExtended) R.r = mg->rExt + (long long)mg->lv[0].nx * mg->lv[0].ny;
        st = cg_solve(R, iteration, residual, residualTrace, traceCapacity);
        if (rExtended && countForDevice > 0) {
            analysis_note_write(rVector->data, sizeof(double) * (size_t)countForDevice);
            if (!MGCG_HIP(hipMemcpyAsync(rVector->data, R.r, sizeof(double) * (size_t)countForDevice, hipMemcpyDeviceToDevice, R.ws->stream)) || !MGCG_HIP(hipStreamSynchronize(R.ws->stream))) st = MGCG_ERROR;
        }
    });
    return st;
}

int SolveMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
            Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
            Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* zVector,
            int elementsCount, int count,
            double allowableResidual, int minIteration, int maxIteration, int rule,
            int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    return SolveMgParallel(nullptr, cublas, cusparse, matDescr, mg, elementsVector, rowOffsetsVector, columnIndecesVector,
                           xVector, bVector, ApVector, pVector, rVector, zVector, count, count, 0, elementsCount, 0, count - 1,
                           allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

// ---------------------------------------------------------------- Jacobi-preconditioned CG for general CSR matrices
// The loop of SolveEx / SolveParallel with z = D^-1 r: alpha = r.z / p.Ap, beta = r.z_new / r.z, p = z + beta p, the stop rules on the
// true residual.  z is element-wise, so it is formed inside the two vector passes (kernels_blas1.hip) and the iteration keeps the plain
// loop's launch count.  The product goes through launch_spmv_auto: compression modes and the automatic column tiles apply unchanged.
// The deferred x update (x_defer) and the placement draw do not apply, as for the V-cycle loop.
int MgcgJacobiSetup(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    int elementsCount, int countForDevice, int offsetForDevice, Vector* dinvVector)
{
    if (!cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector || !dinvVector) { set_error("MgcgJacobiSetup: null handle"); return -1; }
    if (elementsCount < 0 || countForDevice < 0 || offsetForDevice < 0) { set_error("MgcgJacobiSetup: bad sizes"); return -1; }
    if (elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount || rowOffsetsVector->size < (long long)countForDevice + 1) {
        set_error("MgcgJacobiSetup: a device vector is smaller than the matrix"); return -1;
    }
    if (cg_vector_short("MgcgJacobiSetup", "dinv", dinvVector, countForDevice, "local rows")) return -1;
    if (!device_state()) return -1;
    if (countForDevice == 0) return 0;
    hipStream_t s = cusparse->ws.stream;
    int* bad = cusparse->ws.devInts + 6;
    int h2[2] = { 0, 0x7fffffff };
    analysis_note_write(dinvVector->data, sizeof(double) * (size_t)countForDevice);
    bool ok = MGCG_HIP(hipMemcpyAsync(bad, h2, sizeof(h2), hipMemcpyHostToDevice, s));
    if (ok) launch_jacobi_setup(s, elementsVector->data, rowOffsetsVector->data, columnIndecesVector->data, elementsCount, countForDevice, offsetForDevice, dinvVector->data, bad);
    ok = ok && MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(h2, bad, sizeof(h2), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));   // the one read-back
    if (!ok) return -1;
    if (h2[0] == 0) return 0;
    // the failure path: look at the first such row to say what is wrong with it.  These copies go through the null stream, not s: that is
    // correct because s was synchronised just above and the call has enqueued nothing on it since
    const long long row = h2[1];
    int ro[2] = { 0, 0 };
    const char* what = "has no stored diagonal entry";
    double diag = 0.0;
    if (MGCG_HIP(hipMemcpy(ro, rowOffsetsVector->data + row, sizeof(ro), hipMemcpyDeviceToHost))) {
        long long k0 = ro[0] < 0 ? 0 : ro[0], k1 = ro[1] > elementsCount ? elementsCount : ro[1];
        if (k1 <= k0) what = "is empty: it has no stored diagonal entry";
        else {
            std::vector<int> cols((size_t)(k1 - k0));
            if (MGCG_HIP(hipMemcpy(cols.data(), columnIndecesVector->data + k0, sizeof(int) * cols.size(), hipMemcpyDeviceToHost))) {
                for (size_t k = 0; k < cols.size(); ++k) {
                    if (cols[k] != offsetForDevice + row) continue;
                    if (MGCG_HIP(hipMemcpy(&diag, elementsVector->data + k0 + (long long)k, sizeof(double), hipMemcpyDeviceToHost))) what = nullptr;
                    break;
                }
            }
        }
    }
    if (what) set_error("MgcgJacobiSetup: row %lld (local row %lld) %s", (long long)offsetForDevice + row, row, what);
    else set_error("MgcgJacobiSetup: row %lld (local row %lld) has the diagonal %g, which is not finite and > 0 with a finite reciprocal", (long long)offsetForDevice + row, row, diag);
    return -1;
}

int SolveJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                        int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    // A rank whose diagonal set-up failed calls with a null dinvVector: like every other unusable argument it travels in the halo plan's
    // one all-reduce (cg_call), and every rank leaves with MGCG_ERROR.  Null handles are reported before the device is asked for.
    if (!cublas || !cusparse || !dinvVector) {
        set_error("SolveJacobi: null handle");
        if (MgcgCommSize(comm) <= 1) return MGCG_ERROR;
    } else if (!device_state()) return MGCG_ERROR;
    const CgCall c = { "SolveJacobi", comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        if (dinvVector->size < countForDevice) { set_error("SolveJacobi: the dinv vector is smaller than the problem"); return false; }
        return true;
    };
    int st = MGCG_ERROR;
    cg_call(c, dinvVector != nullptr, checks, [&](CgRun& R) {
        R.dinv = dinvVector->data;
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        st = cg_solve(R, iteration, residual, residualTrace, traceCapacity);
    });
    return st;
}

int SolveJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                int elementsCount, int count,
                double allowableResidual, int minIteration, int maxIteration, int rule,
                int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    return SolveJacobiParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                               xVector, bVector, ApVector, pVector, rVector, dinvVector, count, count, 0, elementsCount, 0, count - 1,
                               allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

// Single-reduction CG (cg_solve_sreduce above; refusals: cg_variant_call).  Whether dinvVector is given is NOT part of the ranks' agreement:
// every rank passes one, or none does -- the all-reduce carries three sums or two.
int SolveSingleReduceParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                              Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* sVector, Vector* dinvVector,
                              int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                              double allowableResidual, int minIteration, int maxIteration, int rule,
                              int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "SolveSingleReduce";
    const CgCall c = { who, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        return !cg_rule_refused(who, rule, "the pass carries no max|r|") && !cg_vector_short(who, "s", sVector, countForDevice, "local rows") &&
               !(dinvVector && cg_vector_short(who, "dinv", dinvVector, countForDevice, "local rows"));
    };
    return cg_variant_call(c, cublas && cusparse && sVector, checks, [&](CgRun& R) {
        R.dinv = cg_dinv_address(R, dinvVector);
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.r, R.Ap, sVector->data }, countForDevice);
        cg_note_written({ R.p }, count);
        return cg_solve_sreduce(R, sVector->data, iteration, residual, residualTrace, traceCapacity);
    });
}

int SolveSingleReduce(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* sVector, Vector* dinvVector,
                      int elementsCount, int count,
                      double allowableResidual, int minIteration, int maxIteration, int rule,
                      int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    return SolveSingleReduceParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                                     xVector, bVector, ApVector, pVector, rVector, sVector, dinvVector, count, count, 0, elementsCount, 0, count - 1,
                                     allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

// MINRES (cg_solve_minres above; refusals: cg_variant_call).  The shift is NOT part of the ranks' agreement: every rank passes the same.
int SolveMinresParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* w1Vector, Vector* w2Vector,
                        int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ, double shift,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "SolveMinres";
    const CgCall c = { who, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        if (!(std::fabs(shift) <= 1.79e308)) { set_error("%s: the shift is not finite", who); return false; }
        return !cg_rule_refused(who, rule, "the recurrence carries no max|r|") && !cg_vector_short(who, "w1", w1Vector, countForDevice, "local rows") && !cg_vector_short(who, "w2", w2Vector, countForDevice, "local rows") &&
               !(rVector && cg_vector_short(who, "r", rVector, count, "columns (both Lanczos buffers are full length)"));
    };
    return cg_variant_call(c, cublas && cusparse && w1Vector && w2Vector, checks, [&](CgRun& R) {
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.Ap, w1Vector->data, w2Vector->data }, countForDevice);
        cg_note_written({ R.p, R.r }, count);
        return cg_solve_minres(R, w1Vector->data, w2Vector->data, shift, iteration, residual, trueResidual, residualTrace, traceCapacity);
    });
}

int SolveMinres(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* w1Vector, Vector* w2Vector,
                int elementsCount, int count, double shift,
                double allowableResidual, int minIteration, int maxIteration, int rule,
                int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    return SolveMinresParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                               xVector, bVector, ApVector, pVector, rVector, w1Vector, w2Vector, count, count, 0, elementsCount, 0, count - 1, shift,
                               allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

// LSQR (lsqr_solve above), one rank.  The shapes differ from every other export's, so the refusals are worded here: what needs no device is
// refused before one is asked for, and nothing is enqueued for a call that fails.
int MgcgSolveLsqr(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
              Vector* elementsTVector, VectorInt* rowOffsetsTVector, VectorInt* columnIndecesTVector,
              Vector* xVector, Vector* bVector, Vector* uVector, Vector* vVector, Vector* wVector, Vector* qVector, Vector* tVector,
              int elementsCount, int rows, int columns, double damp,
              double allowableResidual, int minIteration, int maxIteration, int rule,
              int* iteration, double* residual, double* residualNorm, double* trueResidual, double* trueNormalResidual,
              double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "MgcgSolveLsqr";
    if (!cublas || !cusparse) { set_error("%s: null handle", who); return MGCG_ERROR; }
    if (!elementsVector || !rowOffsetsVector || !columnIndecesVector || !elementsTVector || !rowOffsetsTVector || !columnIndecesTVector ||
        !xVector || !bVector || !uVector || !vVector || !wVector || !qVector || !tVector) { set_error("%s: null vector handle", who); return MGCG_ERROR; }
    if (rows < 1 || columns < 1 || elementsCount < 0) { set_error("%s: bad sizes (rows %d, columns %d, elementsCount %d)", who, rows, columns, elementsCount); return MGCG_ERROR; }
    if (!(damp >= 0.0 && damp <= 1.79e308)) { set_error("%s: damp is negative or not finite", who); return MGCG_ERROR; }
    if (cg_rule_refused(who, rule, "the recurrence carries no max-norm of A^T r")) return MGCG_ERROR;
    if (residualTrace && traceCapacity > 0x7ffffff0) { set_error("%s: trace capacity too large", who); return MGCG_ERROR; }
    auto matrix_short = [&](const char* name, const Vector* e, const VectorInt* ro, const VectorInt* ci, int nRows) {
        if (e->size >= elementsCount && ci->size >= elementsCount && ro->size >= (long long)nRows + 1) return false;
        set_error("%s: a vector of %s is smaller than the matrix (%d stored entries, %d rows)", who, name, elementsCount, nRows);
        return true;
    };
    if (matrix_short("A", elementsVector, rowOffsetsVector, columnIndecesVector, rows) ||
        matrix_short("A^T", elementsTVector, rowOffsetsTVector, columnIndecesTVector, columns)) return MGCG_ERROR;
    if (cg_vector_short(who, "x", xVector, columns, "columns") || cg_vector_short(who, "b", bVector, rows, "rows") ||
        cg_vector_short(who, "u", uVector, rows, "rows") || cg_vector_short(who, "v", vVector, columns, "columns") ||
        cg_vector_short(who, "w", wVector, columns, "columns") || cg_vector_short(who, "q", qVector, rows, "rows") ||
        cg_vector_short(who, "t", tVector, columns, "columns")) return MGCG_ERROR;
    if (!device_state()) return MGCG_ERROR;
    CgRun R;
    R.ws = &cublas->ws; R.cusparse = cusparse; R.nLocal = rows; R.count = columns;
    cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
    LsqrMatrix A = { elementsVector->data, rowOffsetsVector->data, columnIndecesVector->data, elementsCount, rows, columns };
    LsqrMatrix At = { elementsTVector->data, rowOffsetsTVector->data, columnIndecesTVector->data, elementsCount, columns, rows };
    const LsqrRun P = { R.ws, xVector->data, uVector->data, vVector->data, wVector->data, qVector->data, tVector->data, bVector->data, rows, columns, damp };
    cg_note_written({ P.uh, P.q }, rows);
    cg_note_written({ P.x, P.vh, P.w, P.t }, columns);
    return lsqr_solve(R, A, At, P, iteration, residual, residualNorm, trueResidual, trueNormalResidual, residualTrace, traceCapacity);
}

// LOBPCG (lob_entry above), one rank: no preconditioner or, with dinvVector, the diagonal's; and with a hierarchy, its cycle
long long MgcgLobpcgWorkSize(int count, int k)
{
    if (count < 1 || k < 1 || k > kBlockMaxK) return 0;
    return 6LL * k * cg_work_stride(count);           // (at most 48 * 2^31: a 64-bit count, as the vectors' sizes are)
}

int MgcgSolveLobpcg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector, Vector* workVector, Vector* dinvVector,
                    int elementsCount, int count, int k, int largest,
                    double allowableResidual, int relative, int minIteration, int maxIteration,
                    int* iteration, double theta[], double residual[], double trueResidual[], int status[], int* restarts,
                    double residualTrace[], int traceCapacity)
{
    (void)matDescr;
    return lob_entry("MgcgSolveLobpcg", false, nullptr, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, workVector, dinvVector,
                     elementsCount, count, k, largest, allowableResidual, relative, minIteration, maxIteration,
                     iteration, theta, residual, trueResidual, status, restarts, residualTrace, traceCapacity);
}

int MgcgSolveLobpcgMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* workVector,
                      int elementsCount, int count, int k, int largest,
                      double allowableResidual, int relative, int minIteration, int maxIteration,
                      int* iteration, double theta[], double residual[], double trueResidual[], int status[], int* restarts,
                      double residualTrace[], int traceCapacity)
{
    (void)matDescr;
    return lob_entry("MgcgSolveLobpcgMg", true, mg, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, workVector, nullptr,
                     elementsCount, count, k, largest, allowableResidual, relative, minIteration, maxIteration,
                     iteration, theta, residual, trueResidual, status, restarts, residualTrace, traceCapacity);
}

// BiCGStab (cg_solve_bicgstab above; refusals: cg_variant_call).  With `jacobi` dinvVector is a handle the export requires, with `vcycle`
// the hierarchy (one rank: the export passes no communicator and the whole matrix).
static int bicgstab_entry(const char* who, bool jacobi, bool vcycle, MgcgMg* mg, MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse,
                          Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                          Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                          Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector, Vector* dinvVector,
                          int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                          double allowableResidual, int minIteration, int maxIteration, int rule,
                          int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    const CgCall c = { who, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        return !cg_rule_refused(who, rule, "the loop carries no max|r|") && !cg_vector_short(who, "v", vVector, countForDevice, "local rows") &&
               !cg_vector_short(who, "t", tVector, countForDevice, "local rows") && !cg_vector_short(who, "rhat", rhatVector, countForDevice, "local rows") &&
               !cg_vector_short(who, "s", sVector, count, "columns (p and s are full length)") &&
               !(jacobi && cg_vector_short(who, "dinv", dinvVector, countForDevice, "local rows")) && !(vcycle && (cg_hierarchy_refused(who, mg, count) || cg_kcycle_refused(who, mg)));
    };
    return cg_variant_call(c, cublas && cusparse && vVector && sVector && tVector && rhatVector && (!jacobi || dinvVector) && (!vcycle || mg), checks, [&](CgRun& R) {
        if (vcycle && R.multi) { set_error("%s: the V-cycle form runs on one rank", who); return (int)MGCG_ERROR; }
        if (jacobi) R.dinv = cg_dinv_address(R, dinvVector);
        if (vcycle) R.mg = mg;
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.Ap, R.r, vVector->data, tVector->data, rhatVector->data }, countForDevice);
        cg_note_written({ R.p, sVector->data }, count);
        return cg_solve_bicgstab(R, who, vVector->data, sVector->data, tVector->data, rhatVector->data, iteration, residual, trueResidual, residualTrace, traceCapacity);
    });
}

int SolveBicgstabParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                          Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                          Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                          Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                          int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                          double allowableResidual, int minIteration, int maxIteration, int rule,
                          int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return bicgstab_entry("SolveBicgstab", false, false, nullptr, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector,
                          xVector, bVector, ApVector, pVector, rVector, vVector, sVector, tVector, rhatVector, nullptr,
                          count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ,
                          allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

int SolveBicgstab(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                  Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                  int elementsCount, int count,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    return SolveBicgstabParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                                 xVector, bVector, ApVector, pVector, rVector, vVector, sVector, tVector, rhatVector, count, count, 0, elementsCount, 0, count - 1,
                                 allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

int SolveBicgstabJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                                Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector, Vector* dinvVector,
                                int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                                double allowableResidual, int minIteration, int maxIteration, int rule,
                                int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return bicgstab_entry("SolveBicgstabJacobi", true, false, nullptr, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector,
                          xVector, bVector, ApVector, pVector, rVector, vVector, sVector, tVector, rhatVector, dinvVector,
                          count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ,
                          allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

int SolveBicgstabJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                        Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector, Vector* dinvVector,
                        int elementsCount, int count,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    return SolveBicgstabJacobiParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                                       xVector, bVector, ApVector, pVector, rVector, vVector, sVector, tVector, rhatVector, dinvVector, count, count, 0, elementsCount, 0, count - 1,
                                       allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

// The V-cycle form (one rank): the Jacobi form's seven work vectors, no z vector.  The hierarchy may come from any matrix.
int SolveBicgstabMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                    Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                    int elementsCount, int count,
                    double allowableResidual, int minIteration, int maxIteration, int rule,
                    int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return bicgstab_entry("SolveBicgstabMg", false, true, mg, nullptr, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector,
                          xVector, bVector, ApVector, pVector, rVector, vVector, sVector, tVector, rhatVector, nullptr,
                          count, count, 0, elementsCount, 0, count - 1,
                          allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

int SolveBicgstabL(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                   Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
                   int ell, int elementsCount, int count,
                   double allowableResidual, int minIteration, int maxIteration, int rule,
                   int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return bicgstabl_call({ "SolveBicgstabL", false, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                            workVector, nullptr, elementsCount, count, allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity }, ell);
}

int SolveBicgstabLJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                         Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                         Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector, Vector* dinvVector,
                         int ell, int elementsCount, int count,
                         double allowableResidual, int minIteration, int maxIteration, int rule,
                         int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return bicgstabl_call({ "SolveBicgstabLJacobi", true, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                            workVector, dinvVector, elementsCount, count, allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity }, ell);
}

int SolveGmres(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
               int m, int orth, int elementsCount, int count,
               double allowableResidual, int minIteration, int maxIteration, int rule,
               int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return gmres_call({ "SolveGmres", false, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                        workVector, nullptr, elementsCount, count, allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity }, m, orth);
}

int SolveGmresJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                     Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                     Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector, Vector* dinvVector,
                     int m, int orth, int elementsCount, int count,
                     double allowableResidual, int minIteration, int maxIteration, int rule,
                     int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return gmres_call({ "SolveGmresJacobi", true, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                        workVector, dinvVector, elementsCount, count, allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity }, m, orth);
}

// The V-cycle form (one rank): flexible GMRES, z_j = M^-1 v_j stored behind the basis.  The hierarchy may come from any matrix.
int SolveGmresMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
                 int m, int orth, int elementsCount, int count,
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    return gmres_call({ "SolveGmresMg", false, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                        workVector, nullptr, elementsCount, count, allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity,
                        true, mg }, m, orth);
}

// Preconditioned MINRES (cg_solve_pminres above; refusals: cg_variant_call).  dinvVector, the hierarchy and zVector are handles the exports
// require.  The shift is NOT part of the ranks' agreement.
static bool pminres_common_checks(const char* who, double shift, int rule, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector, int countForDevice)
{
    if (!(std::fabs(shift) <= 1.79e308)) { set_error("%s: the shift is not finite", who); return false; }
    return !cg_rule_refused(who, rule, "the recurrence carries no max|r|") && !cg_vector_short(who, "r1", r1Vector, countForDevice, "local rows") &&
           !cg_vector_short(who, "w1", w1Vector, countForDevice, "local rows") && !cg_vector_short(who, "w2", w2Vector, countForDevice, "local rows");
}

int SolveMinresJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                              Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                              Vector* dinvVector,
                              int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ, double shift,
                              double allowableResidual, int minIteration, int maxIteration, int rule,
                              int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "SolveMinresJacobi";
    const CgCall c = { who, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        return pminres_common_checks(who, shift, rule, r1Vector, w1Vector, w2Vector, countForDevice) && !cg_vector_short(who, "dinv", dinvVector, countForDevice, "local rows");
    };
    return cg_variant_call(c, cublas && cusparse && r1Vector && w1Vector && w2Vector && dinvVector, checks, [&](CgRun& R) {
        R.dinv = cg_dinv_address(R, dinvVector);
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.Ap, R.r, r1Vector->data, w1Vector->data, w2Vector->data }, countForDevice);
        cg_note_written({ R.p }, count);
        return cg_solve_pminres(R, who, r1Vector->data, w1Vector->data, w2Vector->data, shift, iteration, residual, trueResidual, residualTrace, traceCapacity);
    });
}

int SolveMinresJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                      Vector* dinvVector,
                      int elementsCount, int count, double shift,
                      double allowableResidual, int minIteration, int maxIteration, int rule,
                      int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    return SolveMinresJacobiParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                                     xVector, bVector, ApVector, pVector, rVector, r1Vector, w1Vector, w2Vector, dinvVector, count, count, 0, elementsCount, 0, count - 1, shift,
                                     allowableResidual, minIteration, maxIteration, rule, iteration, residual, trueResidual, residualTrace, traceCapacity);
}

int SolveMinresMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                  Vector* zVector,
                  int elementsCount, int count, double shift,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual, double* trueResidual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "SolveMinresMg";
    const CgCall c = cg_call_one_rank(who, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector, elementsCount, count);
    auto checks = [&] {
        if (!pminres_common_checks(who, shift, rule, r1Vector, w1Vector, w2Vector, count) || cg_vector_short(who, "z", zVector, count, "rows")) return false;
        return !cg_hierarchy_refused(who, mg, count) && !cg_kcycle_refused(who, mg);
    };
    // one rank always: cg_variant_call refuses in front of the device, and cg_call's second look at checks() finds nothing new
    return cg_variant_call(c, cublas && cusparse && mg && r1Vector && w1Vector && w2Vector && zVector, checks, [&](CgRun& R) {
        if (R.multi) { set_error("%s: the V-cycle form runs on one rank", who); return (int)MGCG_ERROR; }
        R.mg = mg; R.z = zVector->data;
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.Ap, R.r, R.p, r1Vector->data, w1Vector->data, w2Vector->data, R.z }, count);
        return cg_solve_pminres(R, who, r1Vector->data, w1Vector->data, w2Vector->data, shift, iteration, residual, trueResidual, residualTrace, traceCapacity);
    });
}

// Chebyshev-preconditioned CG (cg_solve_chebyshev above; refusals: cg_variant_call).  Degree, bounds and whether dinvVector is given are NOT part
// of the ranks' agreement: every rank passes the same.
int SolveChebyshevParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                           Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                           Vector* zVector, Vector* z2Vector, Vector* dVector,
                           int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                           int degree, double lambdaMin, double lambdaMax,
                           double allowableResidual, int minIteration, int maxIteration, int rule,
                           int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    (void)matDescr;
    const char* who = "SolveChebyshev";
    const CgCall c = { who, comm, cublas, cusparse, elementsVector, rowOffsetsVector, columnIndecesVector, xVector, bVector, ApVector, pVector, rVector,
                       count, countForDevice, offsetForDevice, elementsCountForDevice, minJ, maxJ };
    auto checks = [&] {
        if (degree < 1 || degree > 16) { set_error("%s: degree %d, must be 1 .. 16", who, degree); return false; }
        if (!(lambdaMin > 0.0 && lambdaMin < lambdaMax && lambdaMax <= 1.79e308)) { set_error("%s: the bounds (%g, %g) must be finite with 0 < lambdaMin < lambdaMax", who, lambdaMin, lambdaMax); return false; }
        return !cg_rule_refused(who, rule, "the passes carry no max|r|") && !cg_vector_short(who, "z", zVector, count, "columns") && !cg_vector_short(who, "z2", z2Vector, count, "columns") &&
               !cg_vector_short(who, "d", dVector, countForDevice, "local rows") && !(dinvVector && cg_vector_short(who, "dinv", dinvVector, countForDevice, "local rows"));
    };
    return cg_variant_call(c, cublas && cusparse && zVector && z2Vector && dVector, checks, [&](CgRun& R) {
        R.dinv = cg_dinv_address(R, dinvVector);
        cg_set_stop(R, allowableResidual, minIteration, maxIteration, rule);
        cg_note_written({ R.x, R.r, R.Ap, dVector->data }, countForDevice);
        cg_note_written({ R.p, zVector->data, z2Vector->data }, count);
        return cg_solve_chebyshev(R, cheb_plan(degree, lambdaMin, lambdaMax), zVector->data, z2Vector->data, dVector->data, iteration, residual, residualTrace, traceCapacity);
    });
}

int SolveChebyshev(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                   Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                   Vector* zVector, Vector* z2Vector, Vector* dVector,
                   int elementsCount, int count, int degree, double lambdaMin, double lambdaMax,
                   double allowableResidual, int minIteration, int maxIteration, int rule,
                   int* iteration, double* residual, double* residualTrace, int traceCapacity)
{
    return SolveChebyshevParallel(nullptr, cublas, cusparse, matDescr, elementsVector, rowOffsetsVector, columnIndecesVector,
                                  xVector, bVector, ApVector, pVector, rVector, dinvVector, zVector, z2Vector, dVector, count, count, 0, elementsCount, 0, count - 1,
                                  degree, lambdaMin, lambdaMax, allowableResidual, minIteration, maxIteration, rule, iteration, residual, residualTrace, traceCapacity);
}

// *bound = max over the local rows of sum_j |a_ij| (times dinv_i with a dinvVector): Gershgorin's upper bound of the spectrum of A (of D^-1 A).
// One launch pair and one read-back; an empty slice gives 0.  Several ranks take the maximum of their bounds themselves.
int MgcgGershgorinBound(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        int elementsCount, int countForDevice, int offsetForDevice, Vector* dinvVector, double* bound)
{
    if (!cusparse || !elementsVector || !rowOffsetsVector || !columnIndecesVector || !bound) { set_error("MgcgGershgorinBound: null handle"); return -1; }
    if (elementsCount < 0 || countForDevice < 0 || offsetForDevice < 0) { set_error("MgcgGershgorinBound: bad sizes"); return -1; }
    if (elementsVector->size < elementsCount || columnIndecesVector->size < elementsCount || rowOffsetsVector->size < (long long)countForDevice + 1) {
        set_error("MgcgGershgorinBound: a device vector is smaller than the matrix"); return -1;
    }
    if (dinvVector && cg_vector_short("MgcgGershgorinBound", "dinv", dinvVector, countForDevice, "local rows")) return -1;
    *bound = 0.0;
    if (countForDevice == 0) return 0;
    if (!device_state()) return -1;
    hipStream_t s = cusparse->ws.stream;
    double* partials = cusparse->ws.partials;
    double* out = partials + kMaxPartials;
    launch_gershgorin(s, elementsVector->data, rowOffsetsVector->data, elementsCount, countForDevice, dinvVector ? dinvVector->data : nullptr, partials, out);
    double h = 0.0;
    const bool ok = MGCG_HIP(hipGetLastError()) && MGCG_HIP(hipMemcpyAsync(&h, out, sizeof(double), hipMemcpyDeviceToHost, s)) && MGCG_HIP(hipStreamSynchronize(s));   // the one read-back
    if (!ok) return -1;
    *bound = h;
    return 0;
}

} // extern "C"
