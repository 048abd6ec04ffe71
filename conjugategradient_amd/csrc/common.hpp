// Internal declarations shared by the translation units of libMgcgGpu.so.
// gfx950 (MI355X, CDNA4) only: 64-wide wavefronts, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <cmath>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

// Only the C ABI is exported from the shared object (-fvisibility=hidden for everything else).
#pragma GCC visibility push(default)
#include "../../include/MgcgGpu.h"
#pragma GCC visibility pop

namespace mgcg {

constexpr int kWave = 64;
constexpr int kBlock = 256;          // threads per workgroup for every streaming kernel
constexpr int kNumXcd = 8;
constexpr int kNumCu = 256;
constexpr int kMaxGrid = kNumCu * 8; // 8 resident 256-thread workgroups per CU (32 waves/CU)
constexpr int kMaxPartials = kNumCu * 32; // single-wavefront workgroups: up to 32 per CU, one partial sum each
constexpr int kXDeferMax = 8;         // longest group of the deferred x update (MGCG_X_DEFER): directions kept in the ring
constexpr int kXDeferDefault = 8;
constexpr int kBlockMaxK = 8;         // right-hand sides of one block CG call (SolveBlockEx / CsrMVBlock)
constexpr int kShiftMaxK = 8;         // shifts of one multi-shift CG call (SolveShifted)
constexpr int kMaxDevices = 64;
constexpr int kPatMax = 256;         // row-pattern form: distinct rows-as-sequences a matrix may have ...
constexpr int kPatEntries = 2048;    // ... and nPattern * longest row (the table lives in LDS: 12 bytes per entry)
constexpr int kPbTileShift = 14;     // propagation-blocking form (class 5, kernels_pb.hip): tiles of 2^14 columns = 128 KB of x in LDS ...
constexpr int kPbTileWidth = 1 << kPbTileShift;
constexpr int kPbMaxTiles = 1024;    // ... at most this many (16.7 M columns: pass 2 holds a block's piece table in LDS) ...
constexpr int kPbRoundCap = 9088;    // ... and rounds of this many entries of a row block (71 KB of LDS in pass 2)

// fn(K) with the run-time column count k of 1 .. 8 as a compile-time constant (K.value).  The callers have checked the range; anything else takes 8.
template <typename Fn>
inline auto dispatch_k(int k, Fn fn)
{
    static_assert(kBlockMaxK == 8 && kShiftMaxK == 8, "one instantiation per column count");
    switch (k) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    default: return fn(std::integral_constant<int, 8>{});
    }
}

// ---------------------------------------------------------------- errors
void set_error(const char* fmt, ...);
bool hip_ok(hipError_t e, const char* what, const char* file, int line);
#define MGCG_HIP(call) ::mgcg::hip_ok((call), #call, __FILE__, __LINE__)

// ---------------------------------------------------------------- tuning knobs
// Every MGCG_* environment variable the library honours is read ONCE (first use) into this block of atomics; launches read
// the atomics, never the environment (getenv racing a setenv of another thread is undefined, and ranks that read different
// values would take different collective paths).  MgcgSetTuning(name, value) changes one knob for the in-process A/B tools,
// MgcgReloadEnvironment() reads the environment again.  Nothing here changes results: every knob picks between bit-identical
// schedules (include/MgcgGpu.h lists them).
struct Tuning {
    std::atomic<int> overlap{1};             // MGCG_OVERLAP            0 off, 1 where the measured exchange costs more than the hops that hide it, 2 whenever an interior exists
    std::atomic<int> noFold{0};              // MGCG_NO_FOLD            V(1,*): store the first sweep instead of forming it per gather
    std::atomic<int> foldUp{-1};             // MGCG_FOLD_UP            V(1,1): x1 + P e formed per gather of the last sweep instead of a prolongation kernel + stored iterate:
                                             //                         -1 by level size (it pays up to a few ten million rows), 0 never, 1 wherever possible
    std::atomic<int> checkEvery{4};          // MGCG_CHECK_EVERY        iterations the host enqueues ahead of the stop flag
    std::atomic<int> tileShift{0};           // MGCG_TILE_SHIFT         column tiles of 2^shift columns (0: equal-width tiles of ~2.85 MiB of x, the default)
    std::atomic<int> tilePack{1};            // MGCG_TILE_PACK          column tiles with 12-byte entries (0: the 16-byte form)
    std::atomic<int> autoTiles{1};           // MGCG_AUTO_TILES         Solve-family calls build the column tiles themselves for matrices without locality
    std::atomic<int> verbose{0};             // MGCG_VERBOSE            errors also go to stderr
    std::atomic<int> virtualDevices{0};      // MGCG_VIRTUAL_DEVICES    one physical GPU shown as n devices (tests)
    std::atomic<int> haloStream{0};          // MGCG_HALO_STREAM        overlap schedule: 0 (default) the interior rows on the side stream, every RCCL call on the main stream;
                                             //                         1 the halo exchange on the side stream, all rows on the main stream (measured faster on one GPU, solver.hip;
                                             //                         opt-in until RCCL on two streams of one communicator has run on real multi-GPU hardware)
    std::atomic<int> forceMultiRank{0};      // MGCG_FORCE_MULTIRANK    a one-rank communicator takes the several-ranks code path (measurement)
    std::atomic<int> placement{3};           // MGCG_PLACEMENT          Solve-family calls on >= 32 M-entry p: time the SpMV on this many EXTRA allocations of p and keep the fastest (0: off)
    std::atomic<int> deepHalo{1};            // MGCG_DEEP_HALO          row-partitioned V(1,1): one exchange of a few planes of the right-hand side per coarse level and the sweeps
                                             //                         recomputed on those planes (4 exchanges per MGCG iteration), 0: one exchange per sweep (8)
    std::atomic<int> dotOrder{0};            // MGCG_DOT_ORDER          validation only: 1 = every dot product adds its rounded products strictly left to right and the ranks'
                                             //                         sums in rank order, as the reference's CPU twin does (LongVector.cs:15-31, resultsDot.Sum()) -- traces and
                                             //                         iterates then EQUAL the oracle's; ~0.5 s per 1.3e8-entry dot, never on a timed path
    std::atomic<int> failCommInit{0};        // MGCG_FAIL_COMM_INIT     tests only: MgcgCommInitAll / MgcgCommInitRank report failure (what a host without a working RCCL does)
    std::atomic<int> xDefer{kXDeferDefault}; // MGCG_X_DEFER            one-rank plain CG loop: x += alpha p applied once per group of this many iterations from a ring of
                                             //                         p buffers (1: every iteration; at most kXDeferMax)
};
Tuning& tuning();
void tuning_reload();

// ---------------------------------------------------------------- per-device state
// One stream per device, shared by every handle created on that device, so calls made through
// different handles stay ordered exactly as they are on the reference's default stream.
struct DeviceState {
    int device = -1;
    hipStream_t stream = nullptr;
    int numCu = kNumCu;
};
DeviceState* device_state();   // for the calling thread's current device (lazily created)
int current_device();
bool select_device_only();       // hipSetDevice for the calling thread's device; creates nothing

// The HIP runtime loads a translation unit's code object on the first launch of any of its kernels (1-9 ms each here: 12 ms
// in all, which would land inside the first timed Solve -- a third of the reference driver's 200 iterations).  Asking for a
// kernel's attributes forces the load; device_state() does that once per device for every translation unit of the library.
inline void preload_code_object(const void* kernel) { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, kernel); }
void preload_ops(); void preload_solver(); void preload_comm(); void preload_kernels_spmv(); void preload_kernels_rows();
void preload_kernels_rowtile(); void preload_kernels_dcsr(); void preload_kernels_tiled(); void preload_kernels_blas1();
void preload_kernels_mg(); void preload_kernels_amg(); void preload_spectrum(); void preload_kernels_pb(); void preload_kernels_block(); void preload_kernels_shift();
void preload_kernels_bkrylov(); void preload_kernels_mixed(); void preload_kernels_sreduce(); void preload_kernels_cheb(); void preload_kernels_minres(); void preload_kernels_pminres();
void preload_kernels_bicgstab(); void preload_kernels_bicgstabl(); void preload_kernels_gmres(); void preload_kernels_lsqr(); void preload_kernels_lobpcg();

// Device scalars of one CG run (lives in the handle's workspace).
struct CgScalars {
    double rr;        // r.r  (or r.z for the preconditioned loop) of the previous iteration
    double pAp;
    double rrNew;     // r.r of this iteration (stop test)
    double rzNew;     // r.z of this iteration (preconditioned loop)
    double residual;
    double rr0;
    double nrmInf;
    double beta;
    double alpha;
    int iteration;    // index of the iteration being executed
    int done;         // set by the finalisation kernel; every later kernel exits at once
    int status;
    int pad;          // "x pending": set by the finalisation kernel for update_xp, cleared when no iteration ran
    // Copy of {rr, rr0, alpha, iteration, done} taken by update_r for the x/p update that also finalises the iteration
    // (single rank, no preconditioner): that kernel's workgroups read these while its first workgroup rewrites the live fields
    double fRr, fRr0, fAlpha;
    int fIteration, fDone;
    // Deferred x update (MGCG_X_DEFER > 1): the alphas of the group's earlier iterations, by position in the group, and the ring slot that
    // holds p after the iteration that stopped the loop (0: the caller's buffer)
    double alphaRing[kXDeferMax];
    int pSlot, pad2;
};

static_assert(offsetof(CgScalars, rzNew) == offsetof(CgScalars, rrNew) + sizeof(double), "{rrNew, rzNew} are all-reduced as one pair");

// What the host polls (pinned, device-written).
struct HostMirror {
    volatile double residual;
    volatile int iteration;
    volatile int done;
    volatile int status;
    volatile int pad;
};

// Per-column scalars of the multi-shift loop (SolveShifted, kernels_shift.hip).  The state of the recurrences is kept twice: iteration k
// reads st[k & 1] in every workgroup of its fused pass while that pass's first workgroup writes st[(k + 1) & 1], so no workgroup can see
// a half-written state and no scalar launch of its own is needed.
struct ShiftState {
    double zeta[kShiftMaxK], zetaPrev[kShiftMaxK];   // zeta_k, zeta_{k-1} per column
    double alphaPrev, betaPrev;                      // alpha_{k-1}, beta_{k-1} of the base recurrence
    int live[kShiftMaxK];                            // 1: the column has not stopped
};
struct ShiftScalars {
    double sigma[kShiftMaxK];
    ShiftState st[2];
    double residual[kShiftMaxK];                     // what the caller gets back, written in the column's stopping iteration
    int iteration[kShiftMaxK], status[kShiftMaxK];
};

// What the mixed-precision loop (SolveMixed, kernels_mixed.hip) keeps next to CgScalars.  The live fields are written by the first workgroup
// of the x/p pass or of the restart pass; the r pass freezes what the passes behind it read in every workgroup (fMaxrr, fWant, fBroken),
// as it does with CgScalars' own frozen copies.
struct MixedScalars {
    double maxrr, fMaxrr;    // largest r.r since the last reliable update
    int want, fWant;         // a reliable update is due at the next slot
    int gate;                // what the update's three launches look at: nonzero = skip (closed by every r pass, opened by the x/p pass of a slot)
    int updates;             // reliable updates done
    int fBroken;             // p.Ap of this iteration is not finite and > 0
    int pad;
};

// What the single-reduction loop (SolveSingleReduce*, kernels_sreduce.hip) carries from one body to the next.  Body k reads st[k & 1] in every
// workgroup of its pass while that pass's first workgroup writes st[(k + 1) & 1], as ShiftState does.  red: several ranks only -- this rank's
// {delta, rr, gamma} ({delta, rr} without dinv), all-reduced in place between the launch that writes them and the pass that reads them.
struct SreduceScalars {
    double red[3];
    struct State { double gamma, alpha; } st[2];     // gamma and alpha of the body before
};

// What the MINRES loop (SolveMinres*, kernels_minres.hip) carries from one body to the next.  Body k reads st[k & 1] in every workgroup of its
// two passes while the second pass's first workgroup writes st[(k + 1) & 1], as SreduceScalars does.  red: {delta, y.y, the closing r.r} --
// delta is left there by the first pass for the second (one rank) or all-reduced in place (several ranks, y.y too).  fDone: CgScalars::done
// as the first pass of a body found it; the second pass, which raises `done` itself while its other workgroups may still start, looks here.
// The preconditioned loop (SolveMinresJacobi*, SolveMinresMg; kernels_pminres.hip) uses the same block: red = {v.q, v.v, the closing r.r, r.z, the
// first r.z as the start found it} -- {v.q, v.v} adjacent, so that they travel in one all-reduce of two doubles -- and State::oldb, the beta
// of the body before (the plain loop neither reads nor writes it).
struct MinresScalars {
    double red[5];
    int fDone, pad;
    struct State { double beta, cs, sn, dbar, eps, phibar, oldb; } st[2];
};

// What the BiCGStab loop (SolveBicgstab*, kernels_bicgstab.hip) keeps on the device.  red: {sigma, theta, tau, rr, rhon, the closing r.r} -- several
// ranks only for the first five, all-reduced in place; {theta, tau} and {rr, rhon} are adjacent, so that each pair travels in one all-reduce of
// two doubles.  alpha is written by pass S and omega by pass X, each by its first workgroup, for the passes behind it.  rho: body k reads
// rho[k & 1] in every workgroup of pass S and pass P while pass P's first workgroup writes rho[(k + 1) & 1], as SreduceScalars does.  fDone:
// CgScalars::done as pass S found it; pass X and pass P look here, since pass P raises `done` itself.  brokeS, brokeX: the breakdown of sigma
// (pass S) or omega (pass X), read by later launches only.
struct BicgstabScalars {
    double red[6];
    double alpha, omega;
    double rho[2];
    int fDone, brokeS, brokeX, pad;
};

// What the BiCGStab(l) loop (SolveBicgstabL, SolveBicgstabLJacobi; kernels_bicgstabl.hip) keeps on the device.  rho: step j of body k reads
// rho[k & 1][j] in every workgroup of pass R_j, pass U_j (j > 0) reads rho[k & 1][j - 1] while its first workgroup writes rho[k & 1][j], and pass P
// reads rho[k & 1][l - 1] while its first workgroup writes rho[(k + 1) & 1][0]: no workgroup reads an entry that a workgroup of the same launch
// writes.  alpha is written by pass R_j and omega by the combine pass, each by its first workgroup, for the launches behind it.  fDone:
// CgScalars::done as pass R_0 found it; every later pass of the body looks here, since pass P raises `done` itself.  broke[j]: the breakdown of
// sigma or alpha in pass R_j, cleared by pass R_0 and read by later launches only (pass R_j looks at broke[0 .. j-1]).  early[j]: pass U_j found
// that r_0 as step j - 1 left it meets the stop test -- the body ends there, with rrEarly as its r_0.r_0; the same discipline.  gamma, pivots: what the combine pass solved, for whoever reads the block back.
// red: the closing r.r.
constexpr int kBicgstablMaxL = 4;
constexpr int kBicgstablGram = kBicgstablMaxL * (kBicgstablMaxL + 3) / 2;   // the entries Z_ab, a = 1 .. l, b = 0 .. a
struct BicgstablScalars {
    double red;
    double alpha, omega;
    double rho[2][kBicgstablMaxL];
    double gamma[kBicgstablMaxL];
    double rrEarly;
    int fDone, pivots;
    int broke[kBicgstablMaxL], early[kBicgstablMaxL];
};

// What the GMRES(m) loop (SolveGmres, SolveGmresJacobi; kernels_gmres.hip) keeps on the device.  h: the new column of the Hessenberg matrix as the
// fold launches left it (hp: the h' of the orthogonalisation pass in flight); R, cs, sn, g: the triangular factor (R[i][j], i <= j), the rotations
// and the rotated right-hand side of the cycle, written by pass N's first workgroup; gLast: g_j where pass N of step k looks for it
// (gLast[k & 1]) and writes its successor (gLast[(k + 1) & 1]); cols: the completed columns of the cycle, yCount and y: what the close's first
// launch solved for its x launches.  fDone: CgScalars::done as the first launch of a step found it; note: a restart found r.r zero (1) or not
// finite (2), read by later launches only.  red: the closing r.r.
constexpr int kGmresMaxM = 32;
struct GmresScalars {
    double red;
    double h[kGmresMaxM], hp[kGmresMaxM];
    double cs[kGmresMaxM], sn[kGmresMaxM], g[kGmresMaxM], y[kGmresMaxM];
    double gLast[2];
    double R[kGmresMaxM][kGmresMaxM];
    int fDone, note, cols, yCount;
};

// What the LSQR loop (MgcgSolveLsqr, kernels_lsqr.hip) keeps on the device.  alpha, beta: the norms of the unnormalised vectors vh and uh that the
// body about to run finds; phibar, rhobar, psi2 (the damped residual's sum of psi^2), tr (theta / rho of the body before, for the deferred w
// update): the rotation's state.  Only the start and the scalar launch write them, so no pass reads a field that a workgroup of the same
// launch writes.  rot: what pass V's first workgroup leaves for the scalar launch.  fDone: CgScalars::done as pass U found it; pass V looks
// here, since it raises `done` itself on a breakdown.  bb: b.b; note: what the start refused (0 nothing, 1 beta1, 2 alpha1, 3 g0^2); resNorm:
// the estimate sqrt(phibar^2 + psi2) of the last judged body; red: the closing r.r and t.t.
struct LsqrScalars {
    double red[2];
    double alpha, beta, phibar, rhobar, psi2, tr;
    double bb, resNorm;
    struct Rotation { double betan, rho, c, s, phibarn, psi2; } rot;
    int fDone, note;
};

// ---------------------------------------------------------------- handles
struct BlockScalars;                 // per-column scalars of the block CG loop (kernels_block.hip)
struct LobScalars;                   // the dense problem and per-column results of the LOBPCG loop (kernels_lobpcg.hip)
struct BkScalars;                    // k x k matrices and per-column results of the shared-subspace block CG loop (kernels_bkrylov.hip)
struct Workspace {
    int device = -1;
    hipStream_t stream = nullptr;
    double* partials = nullptr;      // 3 * kMaxPartials doubles: per-workgroup partial sums (SpMV dot | max-norm | r.r of the fused single-rank path)
    CgScalars* scalars = nullptr;    // device
    HostMirror* mirror = nullptr;    // pinned host, device-visible
    double* hostScalar = nullptr;    // pinned host, 4 doubles (Dot results)
    int* devInts = nullptr;          // device, 8 ints (small integer results: far band, longest row, sampled distance; a 64-bit checksum in [4..5])
    double* trace = nullptr;         // device residual trace
    int traceCap = 0;
    // the library-owned slots 1 .. kXDeferMax-1 of the deferred x update's ring of p (slot 0 is the caller's p), ringSize entries each
    double* ring[kXDeferMax] = {};
    long long ringSize = 0;
    // block CG (kernels_block.hip), allocated at its first call and kept: 3 regions of kBlockMaxK * kMaxPartials partial sums, one
    // region per column of kMaxPartials doubles, and the per-column scalars
    double* blockPartials = nullptr;
    BlockScalars* blockScalars = nullptr;
    ShiftScalars* shiftScalars = nullptr;        // multi-shift CG (kernels_shift.hip), allocated at its first call and kept
    // shared-subspace block CG (kernels_bkrylov.hip), allocated at its first call and kept: 36 regions of kMaxPartials partial sums, one per
    // entry of the upper triangle of an 8 x 8 Gram matrix, and the loop's small matrices
    double* gramPartials = nullptr;
    BkScalars* bkScalars = nullptr;
    // mixed-precision CG (kernels_mixed.hip), allocated at its first call and grown when a larger system comes: the loop's scalars and the four
    // fp32 work vectors xs, r32, p32, Ap32, each mixedStride floats from the last (a multiple of 4: every vector starts on a 16-byte boundary)
    MixedScalars* mixedScalars = nullptr;
    float* mixedVecs = nullptr;
    long long mixedStride = 0;
    SreduceScalars* sreduceScalars = nullptr;    // single-reduction CG (kernels_sreduce.hip), allocated at its first call and kept; its direction p takes ring[1]
    MinresScalars* minresScalars = nullptr;      // MINRES (kernels_minres.hip), allocated at its first call and kept
    BicgstabScalars* bicgstabScalars = nullptr;  // BiCGStab (kernels_bicgstab.hip), allocated at its first call and kept
    // BiCGStab(l) (kernels_bicgstabl.hip), allocated at its first call and kept: the loop's scalars, and kBicgstablGram + 2 regions of kMaxGrid
    // partial sums -- one per entry Z_ab of the Gram pass, then r.r and rtilde.r of the combine pass
    BicgstablScalars* bicgstablScalars = nullptr;
    double* bicgstablPartials = nullptr;
    // GMRES(m) (kernels_gmres.hip), allocated at its first call and kept: the loop's scalars, and kGmresMaxM + 1 regions of kMaxGrid partial
    // sums -- one per column of the basis for v_i.w, then w.w (and every r.r of the loop)
    GmresScalars* gmresScalars = nullptr;
    double* gmresPartials = nullptr;
    LsqrScalars* lsqrScalars = nullptr;          // LSQR (kernels_lsqr.hip), allocated at its first call and kept
    // LOBPCG (kernels_lobpcg.hip), allocated at its first call and kept: the loop's scalars and three regions of Gram partial sums
    LobScalars* lobScalars = nullptr;
    double* lobPartials = nullptr;
    bool init();
    void destroy();
    bool ensure_trace(int cap);
    bool ensure_ring(int slots, long long n);    // slots 1 .. slots-1 allocated with >= n entries (keeps what is there)
    void free_ring();
    bool ensure_block();                         // blockPartials / blockScalars (kernels_block.hip)
    bool ensure_shift();                         // shiftScalars (kernels_shift.hip)
    bool ensure_bkrylov();                       // gramPartials / bkScalars (kernels_bkrylov.hip)
    bool ensure_mixed(long long n);              // mixedScalars / mixedVecs for n rows (kernels_mixed.hip)
    bool ensure_sreduce();                       // sreduceScalars (kernels_sreduce.hip)
    bool ensure_minres();                        // minresScalars (kernels_minres.hip)
    bool ensure_bicgstab();                      // bicgstabScalars (kernels_bicgstab.hip)
    bool ensure_bicgstabl();                     // bicgstablScalars / bicgstablPartials (kernels_bicgstabl.hip)
    bool ensure_gmres();                         // gmresScalars / gmresPartials (kernels_gmres.hip)
    bool ensure_lsqr();                          // lsqrScalars (kernels_lsqr.hip)
    bool ensure_lobpcg();                        // lobScalars / lobPartials (kernels_lobpcg.hip)
};

} // namespace mgcg

struct MgcgBlas   { mgcg::Workspace ws; };
namespace mgcg {
// Dictionary-compressed CSR (kernels_dcsr.hip): what the kernel sees ...
struct DcsrView {
    const unsigned char* colCode;    // code of (col - row) per nonzero
    const unsigned char* valCode;    // code of the value per nonzero, or nullptr (values stay fp64 in `elements`)
    const int* deltaDict;
    const double* valueDict;
    int nDelta, nValue;
    long long rowBase;               // global index of local row 0
    // row-pattern form (class 3): one byte per ROW names the row's whole (offsets, values) sequence
    const unsigned char* patternId;  // nullptr: not in pattern form
    const int* patCount;             // [nPattern] entries per pattern
    const int* patDelta;             // [nPattern * patWidth]
    const double* patValue;          // [nPattern * patWidth]
    int nPattern, patWidth;
    // column-tiled form (class 4): nonzeros re-laid out by column tile, row-major inside a tile
    const double* tileVals;          // nullptr: not tiled; else the nonzeros in tile-major, row-major order ...
    const int* tileCols;             // ... their column ids ...
    const int* tileRowIds;           // ... and (local) row ids
    const int* tileStartHost;        // HOST array [nTiles + 1]: first entry of every tile
    // 12-byte entries (the default when the row ids fit): tilePacked[k] = column offset inside the tile (low tileShift bits) | row - base row
    // of the entry's block of 1024 (high bits); tileHdr[b] = { base row, row of the entry in front of the block or -1 }, blocks numbered
    // tile by tile from tileHdrBaseHost[t]; tileCols / tileRowIds are then not kept
    const unsigned* tilePacked;
    const int2* tileHdr;
    const int* tileHdrBaseHost;      // HOST array [nTiles]: first header of the tile, or -1 for a tile that keeps 16-byte entries (its row ids do not fit)
    int tileShift;
    int tileWidth;                   // columns per tile (equal-width tiles, <= 2^tileShift)
    int nTiles;
    long long tileRows;              // rows of the analysed matrix
    // propagation-blocking form (class 5, kernels_pb.hip explains the layout): pbVals != nullptr says the form exists
    const double* pbVals;
    const unsigned short* pbCols;
    const unsigned short* pbPos;
    double* pbProd;                  // the products of pass 1 (scratch of every product through this form)
    const unsigned* pbPiece;
    const int* pbTileStart;
    const unsigned* pbPieceOff;
    const int* pbRoundOff;
    const unsigned short* pbRowBounds;
    int pbTiles, pbBlocks;
    long long pbColumns;             // length of x the form was built for
};
// ... and what the handle caches per analysed matrix (keyed by the CSR pointers and sizes).
struct DcsrMatrix {
    const double* elements = nullptr; const int* rowOffsets = nullptr; const int* columnIndeces = nullptr;
    long long rows = 0, nnz = 0, rowBase = 0;
    unsigned char* colCode = nullptr; unsigned char* valCode = nullptr;
    int* deltaDict = nullptr; double* valueDict = nullptr;
    int nDelta = 0, nValue = 0;
    unsigned char* patternId = nullptr; int* patCount = nullptr; int* patDelta = nullptr; double* patValue = nullptr;
    int nPattern = 0, patWidth = 0;
    double* tileVals = nullptr; int* tileCols = nullptr; int* tileRowIds = nullptr; int nTiles = 0; long long tileRows = 0;
    unsigned* tilePacked = nullptr; int2* tileHdr = nullptr; int tileShift = 0, tileWidth = 0;
    std::vector<int> tileStart, tileHdrBase;
    double* pbVals = nullptr; unsigned short* pbCols = nullptr; unsigned short* pbPos = nullptr; double* pbProd = nullptr; unsigned* pbPiece = nullptr;
    unsigned* pbPieceOff = nullptr; int* pbTileStart = nullptr; int* pbRoundOff = nullptr; unsigned short* pbRowBounds = nullptr;
    int pbTiles = 0, pbBlocks = 0, pbMaxRounds = 0; long long pbColumns = 0;
    unsigned long long checksum = 0;  // of the CSR arrays the analysis was made from (forms chosen without the caller asking are re-verified per solve)
    int trustedUses = 0;              // per-op products served from this form since its checksum was last verified (dcsr_lookup_op: re-verified every 16th)
    bool automatic = false;           // built by the library's own choice (column tiles for a matrix without locality), not by MgcgSetMatrixCompression
    bool usable = false;
    std::atomic<bool> stale{false};   // a write through the library touched the arrays the analysis was made from: analyse again at the next use
    void release();
    DcsrView view() const
    {
        DcsrView v; v.colCode = colCode; v.valCode = valCode; v.deltaDict = deltaDict; v.valueDict = valueDict; v.nDelta = nDelta; v.nValue = nValue; v.rowBase = rowBase;
        v.patternId = patternId; v.patCount = patCount; v.patDelta = patDelta; v.patValue = patValue; v.nPattern = nPattern; v.patWidth = patWidth;
        v.tileVals = tileVals; v.tileCols = tileCols; v.tileRowIds = tileRowIds; v.tileStartHost = tileStart.data(); v.nTiles = nTiles; v.tileRows = tileRows;
        v.tilePacked = tilePacked; v.tileHdr = tileHdr; v.tileHdrBaseHost = tileHdrBase.data(); v.tileShift = tileShift; v.tileWidth = tileWidth;
        v.pbVals = pbVals; v.pbCols = pbCols; v.pbPos = pbPos; v.pbProd = pbProd; v.pbPiece = pbPiece; v.pbTileStart = pbTileStart; v.pbRoundOff = pbRoundOff;
        v.pbPieceOff = pbPieceOff; v.pbRowBounds = pbRowBounds; v.pbTiles = pbTiles; v.pbBlocks = pbBlocks; v.pbColumns = pbColumns;
        return v;
    }
};
// Optional per-launch timing of the SpMV inside the CG loop (bench.py's roofline figure).
struct SpmvProfile {
    bool enabled = false;
    std::vector<hipEvent_t> start, stop;
    int used = 0;
};
}
struct MgcgSparse {
    mgcg::Workspace ws;
    mgcg::SpmvProfile prof;
    int kernel = 0;          // 0 auto
    int rowsPerBlock = 64;
    int flags = 0;           // bit0 nt loads, bit1 xcd-contiguous mapping, bit2 banded schedule (periodRows)
    int gridBlocks = 0;
    int periodRows = 0;      // rows between strongly coupled windows (a grid plane); 0 = unknown
    int tileRows = 0, tilePlanes = 0;   // banded schedule tile (0 = default)
    int analysedMode = 0;               // the compression mode the cached analyses were built under
    int compression = 0;                // opt-in: 0 off, 1 best lossless compact form (row patterns, else per-nonzero codes, else column tiles), 2 per-nonzero codes only,
                                        // 3 as 1 with the propagation-blocking form before the column tiles
    std::vector<mgcg::DcsrMatrix*> analysed;
    // far-band distance found per matrix (the tile order of the row-tile kernel; any value gives the same results, so a stale
    // entry can only cost locality): keyed by the array pointers and the row count
    struct PeriodEntry { const int* rowOffsets; const int* columnIndeces; long long rows, rowBase; int period; int maxRow; long long meanDistance;
                         int products = 0, threshold = 8; };   // per-op calls on this matrix since the column tiles were last (re)built / products before the next build
    std::vector<PeriodEntry> periods;
};
struct MgcgMatDescr { int type = 0; int base = 0; };
struct Vector    { double* data = nullptr; long long size = 0; int device = -1;
                   bool rawExported = false;   // ToRawPtr_Double handed the address out: the library must not move the data any more
                   bool placed = false;        // the placement draw (solver.hip) has looked at this vector
                   int drawCount = 0, drawChosen = -1; float drawMs[16] = {}; };   // ... and what it measured (MgcgLastPlacement)
struct VectorInt { int* data = nullptr;    long long size = 0; int device = -1; };

namespace mgcg {

// ---------------------------------------------------------------- SpMV
enum SpmvEpilogue {
    EPI_AXPBY = 0,   // y = alpha*(A x) + beta*y
    EPI_DOT = 1,     // y = A x ; partial += w_i * y_i
    EPI_RESIDUAL = 2,// y = b - A x
    EPI_JACOBI = 3,  // y = xo + omega*(dinv*(b - A x))
    EPI_RESIDUAL_DOT = 4, // y = b - A x ; partial += y_i*y_i
    EPI_AXPBY_BETA = 5,  // internal: EPI_AXPBY with beta != 0 (reads y)
    EPI_JACOBI_DOT = 6,  // EPI_JACOBI ; partial += b_i * y_i   (last sweep of the V-cycle: r.z of the PCG loop rides along)
    EPI_CHEBYSHEV = 7,   // d = c1*d + c2*(dinv*(b - A x)) ; y = xo + d   (one step of the Chebyshev polynomial preconditioner, kernels_cheb.hip)
    EPI_CHEBYSHEV_DOT = 8 // EPI_CHEBYSHEV ; partial += b_i * y_i   (the polynomial's last step: r.z of the loop rides along)
};
// Timing ablations that produce WRONG results exist only in lab builds of the library (make lab: -DMGCG_LAB).
#ifdef MGCG_LAB
#define MGCG_ABLATE(a, bits) (((a).ablate & (bits)) != 0)
#else
#define MGCG_ABLATE(a, bits) false
#endif
constexpr bool epi_has_dot(int e) { return e == EPI_DOT || e == EPI_RESIDUAL_DOT || e == EPI_JACOBI_DOT || e == EPI_CHEBYSHEV_DOT; }
constexpr bool epi_is_jacobi(int e) { return e == EPI_JACOBI || e == EPI_JACOBI_DOT; }
constexpr bool epi_is_chebyshev(int e) { return e == EPI_CHEBYSHEV || e == EPI_CHEBYSHEV_DOT; }

struct SpmvArgs {
    const double* elements;
    const int* rowOffsets;
    const int* columnIndeces;
    const double* x;
    double* y;
    int elementsCount;
    int rowCount;
    int columnCount;
    double alpha, beta;      // EPI_AXPBY
    const double* w;         // EPI_DOT: weights (own slice of x); EPI_JACOBI / EPI_CHEBYSHEV: xo (own slice of x)
    const double* b;         // EPI_RESIDUAL / EPI_JACOBI / EPI_CHEBYSHEV
    const double* dinv;      // EPI_JACOBI / EPI_CHEBYSHEV
    double omega;            // EPI_JACOBI
    int dinvUniform;         // EPI_JACOBI / EPI_CHEBYSHEV: every diagonal is the same; dinvScalar is used and the dinv array is not read
    double dinvScalar;
    double* d;               // EPI_CHEBYSHEV: the polynomial's increment, one entry per row, read and rewritten by the row's own lane
    double c1, c2;           // EPI_CHEBYSHEV: this step's coefficients
    int xScaled;             // row-pattern and row-tile kernels: the multiplied vector is xOuter * (xInner * x[col]), formed per gather
    double xInner, xOuter;   //   (a first Jacobi sweep from zero folded into the residual pass of the V-cycle)
    // xScaled == 2 (row-tile kernel, Jacobi epilogues): ... + xCoarse[parent(col)] on top -- the piecewise-constant prolongation of the coarse
    // correction folded into the last sweep of a V(1,1) cycle; the sweep's own iterate (w) is formed the same way from b.  The grid has
    // power-of-two nx, ny (lx, ly bits), y / z halved when sy / sz = 1: parent(c) = ((c >> 1) & cM0) | ((c >> cS1) & cM1) | ((c >> cS2) & cM2) with
    // cM0 = nx/2 - 1, cS1 = 1 + sy, cM1 = ((ny >> sy) - 1) << (lx - 1), cS2 = 1 + sy + sz, cM2 = every bit from lx - 1 + ly - sy up
    const double* xCoarse;
    int cM0, cM1, cM2, cS1, cS2;
    int cRowBase;            //   global cell of the launch's row 0 (several ranks / a row range: the sweep's own parent is parent(cRowBase + row))
    double* partials;        // EPI_DOT / EPI_RESIDUAL_DOT / EPI_JACOBI_DOT: one double per workgroup
    const int* doneFlag;     // optional: exit at once when *doneFlag != 0
    int ablate;              // lab builds only (-DMGCG_LAB, tools/spmv_sweep.py --ablate): bit0 skip the y store, bit1 gathers from L1; the product never reads it
};

// Kernel family by average row length (measured on banded and random matrices, profiles/r1/rowlen_sweep.log):
// 10 row-tile "lane = row" form (kernels_rowtile.hip; 9 = its single-wavefront predecessor, kernels_rows.hip),
// 1 row-block stream form, 5 / 6 / 7 = 8 / 16 / 32 lanes per row.
// Validation mode (knob dot_order): every sum in the reference's order -- the lanes-per-row forms add a row's products lane by lane and
// then across lanes (1e-13 from the stored order of SparseMatrix.cs:68-88); the row-block stream form adds them in stored order.
bool dot_reference_order();
inline int spmv_auto_kernel(double avgRow)
{
    if (avgRow <= 8.0) return 10;
    if (avgRow <= 20.0 || dot_reference_order()) return 1;
    if (avgRow <= 28.0) return 5;
    if (avgRow <= 128.0) return 6;
    return 7;
}

// Order in which a lane = row kernel walks its tiles of `tileRows` rows (kernels_rowtile.hip explains the modes).
// gapAt / gapSkip: tiles [gapAt, gapAt + gapSkip) are left out (the enumeration runs over the remaining tiles): the two boundary row
// ranges of a rank's slice in ONE launch while the interior rows between them are multiplied on another stream.
struct TileMap { int mode; int tilesPerPlane; int nPlanes; int per; int gapAt; int gapSkip; };
constexpr int kRowTileRows = 256;    // rows per tile of the row-tile SpMV kernel (kernels_rowtile.hip)
TileMap make_tile_map(long long rows, int periodRows, int nWG, int tileRows);

struct SpmvConfig { int kernel = 0; int rowsPerBlock = 64; int flags = 0; int gridBlocks = 0; int periodRows = 0; int tileRows = 0; int tilePlanes = 0;
                    int maxRow = 0; /* longest row if known (row-tile kernel: 7 gathers per row when <= 7), 0 = unknown */ };

// Launches the SpMV; returns the number of partials written (grid size) for dot epilogues.
int launch_spmv(hipStream_t s, int epilogue, const SpmvArgs& a, const SpmvConfig& cfg);
// Will launch_spmv hand this plain-CSR product to the row-tile kernel?  (the only CSR kernel that can scale x per gather: SpmvArgs::xScaled)
inline bool spmv_takes_rowtile(const SpmvArgs& a, const SpmvConfig& cfg)
{
    int kernel = cfg.kernel;
    if (kernel == 0) kernel = spmv_auto_kernel(a.rowCount > 0 ? (double)a.elementsCount / (double)a.rowCount : 0.0);
    return kernel == 10 && (((uintptr_t)a.elements & 15) == 0) && (((uintptr_t)a.columnIndeces & 15) == 0) && a.elementsCount >= 8 && a.rowCount > 0;
}
// Row-tile kernel for short rows on plain CSR (kernels_rowtile.hip); periodRows = distance of the far band in rows (0: unknown),
// gridReq = wavefronts (0: 8 per CU).  Needs 16-byte aligned elements / columnIndeces and elementsCount >= 8.
int launch_spmv_rowtile(hipStream_t s, int epilogue, const SpmvArgs& a, int periodRows, int gridReq, int maxRow = 0, bool ntWindow = false,
                        int gapAtTile = 0, int gapSkipTiles = 0);
// Distance (in rows) of the farthest band of the matrix, read off one row in the middle of the slice, and the longest row (one pass
// over the row offsets; both remembered per handle -- stale values can only cost speed: any period gives the same results, and rows
// longer than the remembered maximum take the kernel's slow path); the caller's hint (MgcgSetSpmvPeriod) wins for the period.
int spmv_period(MgcgSparse* h, const int* rowOffsets, const int* columnIndeces, long long rows, long long rowBase, int* maxRow = nullptr, long long* meanDistance = nullptr);
void launch_matrix_shape(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long row, long long rowBase, int* out2);
// The same on the dictionary-compressed form of the matrix (a.elements / a.columnIndeces still serve array tails and long rows).
int launch_spmv_rows(hipStream_t s, int epilogue, const SpmvArgs& a, const DcsrView* m, int gridReq, int periodRows = 0);   // m == nullptr: plain CSR; periodRows: z sweep of the row-pattern kernel
bool dcsr_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
                long long rows, long long nnz, long long rowBase, DcsrMatrix* out);
// Row-pattern form: usable (out->patternId != nullptr) when the matrix has <= 256 distinct rows-as-sequences.
bool pattern_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
                   long long rows, long long nnz, long long rowBase, DcsrMatrix* out);
// Column-tiled form: usable (out->tileVals != nullptr) for sorted rows whose entries lie far from the diagonal when x
// (columns doubles) does not fit a few L2s.
bool tiled_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
                 long long rows, long long nnz, long long rowBase, long long columns, DcsrMatrix* out);
int launch_spmv_tiled(hipStream_t s, int epilogue, const SpmvArgs& a, const DcsrView& m);
bool exclusive_scan(hipStream_t s, int* data, long long n);      // in place, n ints whose total fits an int (kernels_tiled.hip)
// Propagation-blocking form (compression mode 3): usable (out->pbVals != nullptr) for rows whose column tiles never step back, a sampled mean
// distance from the diagonal of a tile or more, x of 2 .. kPbMaxTiles tiles, nnz < 2^31 and room on the device.
bool pb_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
              long long rows, long long nnz, long long columns, long long meanDistance, DcsrMatrix* out);
int launch_spmv_pb(hipStream_t s, int epilogue, const SpmvArgs& a, const DcsrView& m);   // whole matrices only; every epilogue, beta != 0 included
// Cached analysis of a matrix on a handle (nullptr: compression off, not applicable, or the build failed).
const DcsrMatrix* dcsr_lookup(MgcgSparse* h, const double* elements, const int* rowOffsets, const int* columnIndeces,
                              long long rows, long long nnz, long long rowBase, long long columns = 0,    // columns: length of x (0: unknown, no column tiling)
                              long long autoMeanDistance = -1,    // >= 0: a Solve-family call; with compression off the library may still build column tiles for a matrix whose entries lie this far (on average) from the diagonal
                              bool trustRegistry = false);        // the three arrays are library-owned vectors: every write the library can see marks the form stale, so no per-call checksum
// Per-op calls (CsrMV, CsrMVDot, Solve0, Solve1: the reference's own phase driver multiplies through these, Mgcg.cu:10-19,116-163): the form
// the caller asked for (MgcgSetMatrixCompression), or -- compression off -- the library's own column tiles for a matrix without locality
// once it has been multiplied a few times through this handle, provided the three arrays are library-owned vectors (Create_*): writes
// through any export mark the form stale (analysis_note_write), so it is trusted without a checksum per call.  Writes by the caller's
// own kernels through ToRawPtr_* pointers are outside the library's view: every 16th product served from the form re-verifies the 64-bit
// checksum of the CSR arrays (0.8 ms per 310 M nonzeros: 2 % of the 16 products), so such a write is noticed within 16 products at the
// latest; a caller that rewrites matrices that way says so with MgcgAnalysisClear, or switches the feature off (MGCG_AUTO_TILES=0).
const DcsrMatrix* dcsr_lookup_op(MgcgSparse* h, const SpmvArgs& a, long long rowBase);
bool vector_owned(const void* p, size_t bytes);   // [p, p + bytes) lies inside a device vector the library allocated
void vector_registry_add(const void* p, size_t bytes);
void vector_registry_remove(const void* p);
unsigned long long csr_checksum(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long rows, long long nnz, unsigned long long* scratch);
// Every export that writes device memory (or frees it) names the range here: analyses made from arrays it overlaps go stale
// and are rebuilt at their next use (the reference re-uploads A into the same vectors on every Initialize():
// Mgcg/cuBlas/Mgcg/ConjugateGradientSingleGpu.cs:134-147).  Costs one relaxed atomic load when nothing is analysed.
void analysis_note_write(const void* p, size_t bytes);
// CSR or compressed, whichever the handle has for this matrix.
int launch_spmv_auto(hipStream_t s, int epilogue, const SpmvArgs& a, const SpmvConfig& cfg, const DcsrMatrix* dc);
// Rows [r0, r1) of the same matrix (a describes the WHOLE local matrix; y, w, b, dinv are shifted here); partials for
// dot epilogues go to `partials`, at most maxGrid of them.
int launch_spmv_range(hipStream_t s, int epilogue, const SpmvArgs& a, const SpmvConfig& cfg, const DcsrMatrix* dc,
                      long long r0, long long r1, double* partials, int maxGrid);

// Rows [0, i0) and [i1, rowCount) -- the boundary rows either side of an interior range -- in ONE launch when the row-tile kernel serves
// the matrix and both cuts fall on its tile boundaries, else in two; partials as launch_spmv_range.
int launch_spmv_two_ranges(hipStream_t s, int epilogue, const SpmvArgs& a, const SpmvConfig& cfg, const DcsrMatrix* dc,
                           long long i0, long long i1, double* partials, int maxGrid);

// ---------------------------------------------------------------- BLAS-1 and fused CG updates
void launch_axpy(hipStream_t s, double* y, const double* x, long long n, double alpha);
void launch_scal(hipStream_t s, double* x, double alpha, long long n);
void launch_xpay(hipStream_t s, double* y, const double* x, long long n, double beta);
void launch_copy(hipStream_t s, double* y, const double* x, long long n);
void launch_fill(hipStream_t s, double* y, double v, long long n);
// knob dot_order: every dot product in the reference's order (one serial sum; the launch_* functions below then return 1 partial)
void launch_dot_serial(hipStream_t s, const double* x, const double* y, long long n, double* out, const int* done,   // out[0] = ((x0 y0 + x1 y1) + x2 y2) + ...
                       const double* w = nullptr);   // w (this kernel only; the Jacobi loop's r.z): the terms become x_i * (w_i * y_i), inner product rounded first
// partials[0..grid) = per-workgroup partial of sum x_i*y_i ; returns grid
int  launch_dot_partials(hipStream_t s, const double* x, const double* y, long long n, double* partials);
int  launch_nrminf_partials(hipStream_t s, const double* x, long long n, double* partials);
// out[0] = sum(partials[0..n)) in a fixed order (mode 0) or max (mode 1)
void launch_reduce(hipStream_t s, const double* partials, int n, double* out, int mode);

// The Jacobi-preconditioned loop (SolveJacobi*) runs the plain loop's start, r update and folded x/p update with dinv != nullptr: z = dinv * r
// is formed inside the passes, never stored, and partialsZ receives the per-workgroup partial sums of r.z next to those of r.r in partials
// (one each under dot_order = 1).  Both are null for the plain loop.
// p = r ; partial r.r      (CG init; with dinv: p = dinv r ; partial r.r and r.z)
int  launch_copy_dot(hipStream_t s, double* p, const double* r, const double* dinv, long long n, double* partials, double* partialsZ, const int* done);
// alpha = sc->rr / sc->pAp ; x += alpha p ; r -= alpha Ap ; partial r.r (and max|r| in partials2 when wantInf)
int  launch_update_xr(hipStream_t s, const CgScalars* sc, double* x, double* r, const double* p, const double* Ap,
                      long long n, double* partials, double* partialsInf);
// the loop's own split: r -= alpha Ap (+ r.r), then x += alpha p and p = z + beta p in one pass over p
// pApPartials != nullptr: p.Ap is still in nPAp per-workgroup partial sums; every workgroup adds them up itself (same fixed
// order everywhere) instead of a separate reduction launch.  partials (output) must not overlap pApPartials.
int  launch_update_r(hipStream_t s, CgScalars* sc, double* r, const double* Ap, const double* dinv, long long n, double* partials, double* partialsZ,
                     double* partialsInf, const double* pApPartials, int nPAp, bool freeze);
void launch_update_xp(hipStream_t s, const CgScalars* sc, double* x, double* p, const double* z, long long n);
// x/p update that first does what finalize_kernel does (every workgroup reduces the r.r partial sums itself and takes the same stop
// decision; workgroup 0 publishes it): one launch fewer per iteration.  Needs update_r launched with freeze = true.
struct FinalizeArgs;
void launch_update_xp_final(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsZ, const double* partialsInf, int nPartials,
                            double* x, double* p, const double* r, const double* dinv, long long n);

// Deferred x update (one rank, no preconditioner): iteration k of a group reads p_k from slot[pos] and writes p_{k+1} to slot[pos + 1],
// or, on the group's last iteration (flush), to slot[0] in place; the flush and the iteration that stops the loop also apply the group's
// pending terms to x, oldest first (x = x + alpha_j p_j, j = slot 0 .. pos).  Same rounded operations in the same order as the x += alpha p
// of every iteration: the same x, bit for bit.
struct RingArgs {
    double* slot[kXDeferMax];
    int pos;        // position of this iteration in its group (= the slot of p_k)
    int flush;      // 1: the group's last iteration
};
void launch_update_xp_ring(hipStream_t s, const FinalizeArgs& f, const double* partials, const double* partialsInf, int nPartials,
                           double* x, const RingArgs& g, const double* z, long long n);
// after a call that may have stopped inside a group: p back into slot 0 when sc->pSlot names another slot
void launch_ring_copy_back(hipStream_t s, const CgScalars* sc, const RingArgs& g, long long n);

// Multi-shift CG (SolveShifted): the fused pass behind update_r (launched with freeze = true) of one base iteration.  It finalises the
// iteration as update_xp_final does, forms every live column's zeta, alpha_j, beta_j and stop decision, and in one pass over r and p does
// p = r + beta p and, per column, x_j += alpha_j p_j and p_j = zeta_j r + beta_j p_j.  x and ps hold k columns of n entries, column j at j * n.
// f.trace: k traces of f.traceCap entries.
void launch_update_shifted(hipStream_t s, int k, const FinalizeArgs& f, ShiftScalars* sh, const double* partials, const double* partialsInf, int nPartials,
                           double* x, double* p, const double* r, double* ps, long long n);

// Block CG (SolveBlockEx; kernels_block.hip has the layout and the kernels).  x, b and r column-major, column j at j * n; p and Ap the row-interleaved
// work blocks.  The loop's stop flag is its own (block_enqueue_snapshot copies it into a pinned int): block_enqueue_start clears it, and every kernel
// of the loop returns at once when it is up.  block_enqueue_start: with MGCG_RULE_SIMPLE x = 0; r = b - A x, p = r and the per-column scalars.  block_enqueue_iteration: the five
// launches of one iteration (seven under dot_order = 1); f carries the stop rule and k traces of f.traceCap entries.
struct BlockRun {
    Workspace* ws;
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    long long n; int k; int rule;
    double* x; const double* b; double *Ap, *p, *r;
};
struct BlockResult { int iteration[kBlockMaxK]; double residual[kBlockMaxK]; int status[kBlockMaxK]; };
bool block_enqueue_start(const BlockRun& R);
bool block_enqueue_iteration(const BlockRun& R, const FinalizeArgs& f);
bool block_read_results(Workspace* ws, BlockResult* out);
void block_enqueue_snapshot(Workspace* ws, volatile int* slot);

// Shared-subspace block CG (SolveBlockKrylov; kernels_bkrylov.hip has the method).  X and B column-major, column j at j * n; S, Q and T the
// row-interleaved work blocks.  The loop's stop flag is ws->scalars->done: bk_enqueue_start expects it cleared, and every kernel of the loop
// returns at once when it is up.  bk_enqueue_start: R = B - A X, its Cholesky factor, Q, S.  bk_enqueue_iteration: the five launches of
// one iteration (seven under dot_order = 1); f carries the stop rule and k traces of f.traceCap entries.
struct BkRun {
    Workspace* ws;
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    long long n; int k;
    double* X; const double* B; double *S, *Q, *T;
};
struct BkResult { int iteration; int failWhich, failPivot; double residual[kBlockMaxK]; int status[kBlockMaxK]; };   // failWhich: 0 none, 1 R0^T R0, 2 S^T A S, 3 W^T W
bool bk_enqueue_start(const BkRun& R);
bool bk_enqueue_iteration(const BkRun& R, const FinalizeArgs& f);
bool bk_read_results(Workspace* ws, int k, BkResult* out);
// T = A S for k interleaved columns with the per-wavefront partial sums of the upper triangle of S^T T, entry e at gramPartials + e * kMaxPartials
// (kernels_block.hip: spmv_block_kernel's gather with the Gram epilogue); returns the number of partial sums per entry
int launch_spmv_block_gram(hipStream_t s, int k, const double* elements, const int* rowOffsets, const int* columnIndeces,
                           const double* S, double* T, long long rows, double* gramPartials, const int* done);

// y_j = A x_j for k columns, x and y column-major with the same column stride ld >= rows (CsrMVBlock's path on operands that lie ld apart);
// done (may be null): a device int, nonzero = the product writes nothing
void launch_spmv_block_plain(hipStream_t s, int k, const double* elements, const int* rowOffsets, const int* columnIndeces,
                             const double* x, double* y, long long ld, long long rows, const int* done);

// LOBPCG (MgcgSolveLobpcg / MgcgSolveLobpcgMg; kernels_lobpcg.hip has the passes and the dense step, include/MgcgGpu.h the method), one rank.
// X: the caller's block, column j at j * n.  AX, W, AW, P, AP, Rv: the six blocks of the work vector, column j of each at j * ld (ld = n
// rounded up to even).  pre: 0 W = R, 1 W = dinv o R inside the residual pass, 2 somebody else forms W from R between lob_enqueue_residual
// and lob_enqueue_rest (the V-cycle).  The loop's stop flag is ws->scalars->done: lob_enqueue_start expects it cleared.
struct LobRun {
    Workspace* ws;
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    long long n, ld; int k, largest, relative, pre;
    double tol; int minIt, maxIt;
    double *X, *AX, *W, *AW, *P, *AP, *Rv; const double* dinv;
    double* trace; int traceCap;
};
struct LobResult {
    int iteration, restarts, failWhich, failPivot;     // failWhich: 0 none, 1 X0^T X0, 2 W^T W (or a zero column of W), 3 the basis [X W], 4 theta, 5 theta of the start block
    double theta[kBlockMaxK], residual[kBlockMaxK], trueResidual[kBlockMaxK]; int status[kBlockMaxK];
};
bool lob_enqueue_start(const LobRun& R);               // AX, the orthonormal start block, its Ritz values
int lob_enqueue_residual(const LobRun& R);             // body: R, its column sums (and W unless pre = 2); returns the partial sums per column
bool lob_enqueue_rest(const LobRun& R, int body, int nR);   // body: the judgement (of nR partial sums), the W step, AW, the Gram matrices, the dense step, the combine pass
bool lob_enqueue_close(const LobRun& R);               // AX = A X once more, R = AX - X theta, the true residuals
bool lob_read_results(Workspace* ws, int k, LobResult* out);

// Mixed-precision CG (SolveMixed; kernels_mixed.hip has the loop and its rounding contract).  e32: the matrix values as floats (MgcgMixedSetup).
// y = A32 x in fp32, every row summed in stored order (lane = row form) or, for long rows outside dot_order = 1, per lane and then across the
// lanes of the row; partials != nullptr: the per-workgroup partial sums of sum (double)x_i (double)y_i ride along (returns their count).
int launch_spmv_float(hipStream_t s, const float* e32, const int* rowOffsets, const int* columnIndeces, const float* x, float* y, long long nnz, long long rows,
                      double* partials, const int* done);
void launch_mixed_convert(hipStream_t s, const double* elements, const int* rowOffsets, long long nnz, long long rows, float* e32, int* flags /* device {inexact, bad, first bad row} */);
struct MixedRun {
    Workspace* ws;
    const float* e32; const int* rowOffsets; const int* columnIndeces;
    long long n, nnz;
    double* x; double* r;
    float *xs, *r32, *p32, *Ap32;
};
// r32 = (float)r, p32 = r32, xs = 0 and the scalars in front of iteration 0 from the nPartials partial sums of r.r in ws->partials
void mixed_enqueue_start(const MixedRun& R, const FinalizeArgs& f, int nPartials);
// the three launches of one iteration (five under dot_order = 1)
bool mixed_enqueue_iteration(const MixedRun& R, const FinalizeArgs& f);
// the first and the last launch of a reliable update; the fp64 residual product goes between them, gated on mixed_gate(R)
void mixed_enqueue_fold(const MixedRun& R);
void mixed_enqueue_restart(const MixedRun& R, const FinalizeArgs& f, int nPartials);
inline const int* mixed_gate(const MixedRun& R) { return &R.ws->mixedScalars->gate; }

// Single-reduction CG (SolveSingleReduce*; kernels_sreduce.hip has the loop).  u: this rank's rows of the full-length buffer the product gathers
// from (without dinv the residual lives there during the loop, and r is not touched); p: the direction; s = A p by recurrence; w = A u.
// given: several ranks -- the sums arrive all-reduced in ws->sreduceScalars->red.  The partial sums of r.r (and of r.u with dinv) of parity q
// live at sreduce_rr_partials(ws, q) (sreduce_gamma_partials): body k reads parity k + 1 and writes parity k, the start writes parity 1.
struct SreduceRun {
    Workspace* ws;
    double *x, *p, *s, *r, *u, *w; const double* dinv;
    long long n; bool given;
};
double* sreduce_rr_partials(Workspace* ws, int parity);
double* sreduce_gamma_partials(Workspace* ws, int parity);
// this rank's sums of body k into ws->sreduceScalars->red, in front of their one all-reduce (nDelta: the product's partial sums in ws->partials)
void sreduce_enqueue_sums(const SreduceRun& R, int k, int nDelta, int nIn);
// the pass of body k; returns the number of partial sums it leaves for body k + 1 (1 under dot_order = 1: two more launches, three with dinv)
int sreduce_enqueue_pass(const SreduceRun& R, const FinalizeArgs& f, int k, int nDelta, int nIn);

// MINRES (SolveMinres*; kernels_minres.hip has the loop, include/MgcgGpu.h the method).  v, vprev: this rank's rows of the two Lanczos buffers
// of body k (the host rotates them; pass A forms y over vprev, pass B vnext over y); w1, w2: the two direction buffers (pass B writes w over
// w1, the host rotates); q = A v.  given: several ranks -- delta and y.y arrive all-reduced in ws->minresScalars->red[0], red[1].
struct MinresRun {
    Workspace* ws;
    double *x, *v, *vprev, *w1, *w2; const double* q;
    long long n; double shift; bool given;
};
double* minres_yy_partials(Workspace* ws);
// r = t + shift x with the partial sums of r.r in minres_yy_partials(ws) (start and closing pass); returns their number (1 under dot_order = 1)
int minres_enqueue_residual(Workspace* ws, const double* t, const double* x, double* r, long long n, double shift);
// the scalars in front of body 0 from those sums (reduceFirst) or from the all-reduced red[1]; r.r not finite or zero stops the loop here
// with MGCG_NONFINITE at iteration 0; then v = r * (1 / beta1) in place
void minres_enqueue_start(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst, double* v, long long n);
// pass A of body k; returns the number of partial sums of y.y it leaves (1 under dot_order = 1: one more launch)
int minres_enqueue_lanczos(const MinresRun& R, int k, int nDelta);
// pass B of body k
void minres_enqueue_update(const MinresRun& R, const FinalizeArgs& f, int k, int nYY);

// Preconditioned MINRES (SolveMinresJacobi*, SolveMinresMg; kernels_pminres.hip has the loop, include/MgcgGpu.h the method).  v: this rank's rows
// of the one full-length buffer (pass B writes the next v over it in place); r1, r2: the two residual buffers of body k (the host rotates them;
// pass A forms rn over r1); w1, w2: the two direction buffers, as in MinresRun; q = A v.  dinv: the Jacobi form -- z = dinv * rn is formed per
// element in both passes; else z: the vector that holds M^-1 rn when pass B runs.  given: several ranks -- {v.q, v.v} and r.z arrive all-reduced
// in ws->minresScalars->red[0 .. 1] and red[3].
struct PminresRun {
    Workspace* ws;
    double *x, *v, *r1, *w1; const double *r2, *w2, *q, *dinv, *z;
    long long n; double shift; bool given;
};
double* pminres_rz_partials(Workspace* ws);
double* pminres_vv_partials(Workspace* ws);
// the start: r = t + shift x and -- dinv given -- the partial sums of r.z, z = dinv * r; returns their number (1 under dot_order = 1; 0 without dinv)
int pminres_enqueue_residual(Workspace* ws, const double* t, const double* x, double* r, const double* dinv, long long n, double shift);
// the scalars in front of body 0 from the partial sums of the first r.z (reduceFirst) or from the all-reduced red[3]; an r.z that is not finite
// and > 0 stops the loop here with MGCG_NONFINITE at iteration 0; then v = z * (1 / beta1) and the partial sums of v.v; returns their number
int pminres_enqueue_start(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst, double* v, const double* r, const double* dinv, const double* z, long long n);
// pass A of body k (nVq, nVv: the partial sums of v.q in ws->partials and of v.v); returns the number of partial sums of r.z it leaves (0 without dinv)
int pminres_enqueue_lanczos(const PminresRun& R, int k, int nVq, int nVv);
// pass B of body k; returns the number of partial sums of v.v it leaves
int pminres_enqueue_update(const PminresRun& R, const FinalizeArgs& f, int k, int nRz);

// BiCGStab (SolveBicgstab*; kernels_bicgstab.hip has the loop, include/MgcgGpu.h the method).  All pointers are this rank's rows.  phat, shat:
// the rows' slices of the two full-length buffers the products gather from; without dinv they ARE p and s (phat == p, shat == s) and nothing
// is stored twice.  With dinv s is written over r (s == r: the two are never alive together) and p lives in a buffer of its own.  v = A phat,
// t = A shat.  given: several ranks -- the sums arrive all-reduced in ws->bicgstabScalars->red.  stored (SolveBicgstabMg, dinv null): the
// vectors are placed as with dinv, but the caller of the passes writes phat and shat itself between them (the V-cycle) -- the start and the
// passes S and P write no hatted copy, pass X reads shat.
struct BicgstabRun {
    Workspace* ws;
    double *x, *r, *p, *s, *phat, *shat, *v, *t, *rhat; const double* dinv;
    long long n; bool given; bool stored;
};
double* bicgstab_tau_partials(Workspace* ws);
double* bicgstab_rr_partials(Workspace* ws);
double* bicgstab_rho_partials(Workspace* ws);
// the start behind r = b - A x: rhat = r, p = r, phat = dinv * r (with dinv; stored: left to the caller) and the partial sums of r.r in bicgstab_rr_partials(ws); returns
// their number (1 under dot_order = 1)
int bicgstab_enqueue_start(const BicgstabRun& R);
// the scalars in front of body 0 from those sums (reduceFirst) or from the all-reduced red[3]; r.r not finite or zero stops the loop here
// with MGCG_NONFINITE at iteration 0
void bicgstab_enqueue_init(Workspace* ws, const FinalizeArgs& f, int nPartials, bool reduceFirst);
// pass S of body k (nSigma: the first product's partial sums of rhat.v in ws->partials): alpha, s, shat
void bicgstab_enqueue_s(const BicgstabRun& R, const FinalizeArgs& f, int k, int nSigma);
// the partial sums of t.t into bicgstab_tau_partials(ws); returns their number (1 under dot_order = 1)
int bicgstab_enqueue_tau(const BicgstabRun& R);
// pass X of body k (nTheta: the second product's partial sums of s.t in ws->partials): omega, x, r and the partial sums of r.r and rhat.r in
// bicgstab_rr_partials(ws) and bicgstab_rho_partials(ws); returns their number, the same for both (1 under dot_order = 1)
int bicgstab_enqueue_x(const BicgstabRun& R, const FinalizeArgs& f, int k, int nTheta, int nTau);
// pass P of body k: the stop decision, beta, p, phat
void bicgstab_enqueue_p(const BicgstabRun& R, const FinalizeArgs& f, int k, int nRr);

// BiCGStab(l) (SolveBicgstabL, SolveBicgstabLJacobi; kernels_bicgstabl.hip has the loop, include/MgcgGpu.h the method), one rank.  r[0 .. l],
// u[0 .. l], rt (the shadow residual) and x: n entries each, 16-byte aligned or not -- the passes take their element-wise form when one is not.
// With dinv `gather` is the one buffer that holds hat(u_j) or hat(r_j) for the next product; without it the products gather from u_j and r_j
// themselves and gather is null.
struct BicgstablRun {
    Workspace* ws;
    int ell;
    double *x, *r[kBicgstablMaxL + 1], *u[kBicgstablMaxL + 1], *rt, *gather; const double* dinv;
    long long n;
};
// the scalars in front of body 0 from the start's nPartials partial sums of r.r in bicgstab_rr_partials(ws) (the start itself is
// bicgstab_enqueue_start: rt = r_0, u_0 = r_0, gather = dinv r_0); r.r not finite or zero stops the loop here with MGCG_NONFINITE at iteration 0
void bicgstabl_enqueue_init(Workspace* ws, const FinalizeArgs& f, int nPartials);
// pass U_j of body k, j = 1 .. l - 1 (nRho: the partial sums of rt.r_j in ws->partials, left by the product that made r_j; nRr: those of r_0.r_0
// that pass R_{j-1} left): the stop test on r_0 in front of the step, beta, u_0 .. u_j, gather = hat(u_j)
void bicgstabl_enqueue_u(const BicgstablRun& R, const FinalizeArgs& f, int k, int j, int nRho, int nRr);
// pass R_j of body k, j = 0 .. l - 1 (nSigma: the partial sums of rt.u_{j+1} in ws->partials): alpha, the breakdown test, r_0 .. r_j, x, gather = hat(r_j)
// and the partial sums of the new r_0.r_0; returns their number (1 under dot_order = 1)
int bicgstabl_enqueue_r(const BicgstablRun& R, const FinalizeArgs& f, int k, int j, int nSigma);
// the Gram pass: the partial sums of Z_ab = r_a.r_b; returns their number per entry (1 under dot_order = 1)
int bicgstabl_enqueue_gram(const BicgstablRun& R);
// the combine pass (nGram: partial sums per entry of Z): gamma, u_0, x, r_0 and the partial sums of r_0.r_0 and rt.r_0; returns their number (1 under dot_order = 1)
int bicgstabl_enqueue_combine(const BicgstablRun& R, const FinalizeArgs& f, int k, int nGram);
// pass P of body k: the stop decision, beta, u_0, gather = hat(u_0)
void bicgstabl_enqueue_p(const BicgstablRun& R, const FinalizeArgs& f, int k, int nRr);

// GMRES(m) (SolveGmres, SolveGmresJacobi; kernels_gmres.hip has the loop, include/MgcgGpu.h the method), one rank.  V: the basis, column i at
// V + i * stride, m + 1 columns; w: the product's output; r: where the start and every restart leave b - A x.  With dinv `gather` is the one
// buffer that holds hat(v_j) for the next product; without it the products gather from v_j itself and gather is null.  The flexible form
// (SolveGmresMg): Z holds z_j = M^-1 v_j, column j at Z + j * stride, m columns, written by the caller's cycles; the products gather from z_j
// and the close adds sum y_i z_i.  Null in the other two forms.
struct GmresRun {
    Workspace* ws;
    int m, orth;
    double *x, *r, *w, *V, *gather; const double* dinv;
    long long stride, n;
    double* Z;
};
// where the start, every restart and the closing product leave the partial sums of r.r
double* gmres_rr_partials(Workspace* ws);
// the scalars in front of step 0 from the start's nPartials partial sums of r.r; r.r not finite or zero stops the loop here with MGCG_NONFINITE
// at iteration 0
void gmres_enqueue_init(const GmresRun& R, const FinalizeArgs& f, int nPartials);
// v_0 = r / sqrt(r.r), gather = dinv v_0 and g_0 for step k, from nRr partial sums; first: the start (judged by gmres_enqueue_init), else an r.r
// that is zero or not finite ends the loop through the next step's pass N
void gmres_enqueue_restart(const GmresRun& R, const FinalizeArgs& f, int k, int nRr, bool first);
// everything of step k (j = k mod m) behind its product: the orthogonalisation passes and pass N
void gmres_enqueue_step(const GmresRun& R, const FinalizeArgs& f, int k, int j);
// the close: y, and x += hat(sum y_i v_i) -- with Z: x += sum y_i z_i -- over the columns the cycle completed; does nothing when there are none
void gmres_enqueue_close(const GmresRun& R);

// LSQR (MgcgSolveLsqr; kernels_lsqr.hip has the loop, include/MgcgGpu.h the method), one rank.  uh (rows) and vh (columns): the two unnormalised
// vectors of the bidiagonalisation; w, x: columns; q = A vh (rows); t = A^T uh (columns); b: rows.
struct LsqrRun {
    Workspace* ws;
    double *x, *uh, *vh, *w, *q, *t; const double* b;
    long long rows, columns; double damp;
};
double* lsqr_uu_partials(Workspace* ws);
double* lsqr_vv_partials(Workspace* ws);
// the start in front of t = A^T uh: x = 0, uh = b, beta1 = sqrt(b.b)
void lsqr_enqueue_start_beta(const LsqrRun& R);
// ... and behind it: vh = t * (1 / beta1), alpha1 = sqrt(vh.vh), g0 = alpha1 beta1 and the scalars in front of body 0; a beta1 or alpha1 that is
// zero or not finite stops the loop here with MGCG_NONFINITE at iteration 0
void lsqr_enqueue_start_alpha(const LsqrRun& R, const FinalizeArgs& f);
// pass U of body k behind q = A vh; returns the number of partial sums of uh.uh it leaves (1 under dot_order = 1: one more launch)
int lsqr_enqueue_u(const LsqrRun& R, int k);
// pass V of body k behind t = A^T uh, and the scalar launch (under dot_order = 1 one more launch between them)
void lsqr_enqueue_v(const LsqrRun& R, const FinalizeArgs& f, int k, int nUU);
// the close: the partial sums of r.r of r = b - A x in uh -> lsqr_uu_partials; t = t - damp^2 x and those of t.t -> lsqr_vv_partials; each
// returns their number (1 under dot_order = 1)
int lsqr_enqueue_close_residual(const LsqrRun& R);
int lsqr_enqueue_close_normal(const LsqrRun& R);

// Chebyshev-preconditioned CG (SolveChebyshev*; kernels_cheb.hip has the method, solver.hip's cg_solve_chebyshev the loop).
// The start: d = it * (dinv r), z = d, the partial sums of r.r and -- withRz, degree 1 -- of r.z; returns their number (1 under dot_order = 1).
int launch_cheb_start(hipStream_t s, const double* r, const double* dinv, double* d, double* z, long long n, double it,
                      double* partials, double* partialsZ, bool withRz);
// The scalars in front of iteration 0 from those sums (reduceFirst) or from the all-reduced {sc->rrNew, sc->rzNew}; an r.z that is not finite
// and > 0 stops the loop here with MGCG_NONFINITE.
void launch_cheb_init_scalars(hipStream_t s, const double* partials, int n, const double* partialsZ, int nZ, bool reduceFirst, const FinalizeArgs& f);
// The first pass of an iteration: alpha = r.z / p.Ap (pApPartials as launch_update_r; a p.Ap that is not finite and > 0 stops the loop),
// r += (-alpha) Ap, the partial sums of r.r, d = it * (dinv r), z = d and -- withRz -- the partial sums of r.z.
int launch_cheb_first(hipStream_t s, const FinalizeArgs& f, double* r, const double* Ap, const double* dinv, double* d, double* z, long long n, double it,
                      double* partials, double* partialsZ, bool withRz, const double* pApPartials, int nPAp);
// Residual, stop test, the r.z breakdown test, beta and the hand-over of r.z; launch_update_xp follows.
void launch_cheb_finalize(hipStream_t s, const double* partials, int n, const double* partialsZ, int nZ, bool reduceFirst, const FinalizeArgs& f);
// out[0] = max over the rows of sum_k |a_ik| (times dinv_i), each row summed in stored order from +0.0; partials: room for kMaxGrid doubles, out: one more, elsewhere
void launch_gershgorin(hipStream_t s, const double* elements, const int* rowOffsets, long long nnz, long long n, const double* dinv, double* partials, double* out);

// dinv_i = 1 / a_ii for the Jacobi-preconditioned loop
void launch_jacobi_setup(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long nnz, long long n, long long rowBase,
                         double* dinv, int* bad /* device {0, INT_MAX}: {some row failed, the first such row} */);

struct FinalizeArgs {
    CgScalars* sc;
    HostMirror* mirror;
    double* trace; int traceCap;
    double tol; int minIt; int maxIt; int rule;
    int preconditioned;     // 1: beta = rzNew/rr(rz) computed by finalize_precond instead; 2: by this kernel from the all-reduced sc->rzNew
};
// The stop decision of one iteration (the five rules of SURVEY.md 3.5): residual to show, stop or not, status.  Shared by the
// single-vector loop (kernels_blas1.hip) and the block loop (kernels_block.hip); it reads f.rule, f.tol, f.minIt and f.maxIt only.
struct StopDecision { double res, shown; bool stop; int status; };
__device__ __forceinline__ StopDecision decide_stop(const FinalizeArgs& f, double rrNew, double inf, double rr0, int it)
{
    StopDecision d;
    d.res = sqrt(rrNew);
    if (f.rule == MGCG_RULE_HANDMADECL) d.res = inf;
    d.shown = d.res;
    bool converged;
    switch (f.rule) {
    case MGCG_RULE_NATIVE:   converged = (f.minIt <= it) && (d.res < f.tol); break;
    case MGCG_RULE_SIMPLE:   converged = (f.minIt < it) && (d.res < f.tol); break;
    case MGCG_RULE_VIENNACL: d.shown = sqrt(rrNew / rr0); converged = (f.minIt < it) && (rrNew / rr0 < f.tol * f.tol); break;
    default:                 converged = (it >= f.minIt) && (it <= f.maxIt) && (d.res < f.tol); break;  // ConjugateGradient.cs:56-79
    }
    d.status = MGCG_OK;
    d.stop = converged;
    if (!d.stop && it >= f.minIt && it > f.maxIt) { d.stop = true; d.status = MGCG_MAXIT_EXCEEDED; }
    if (!d.stop && !(d.res == d.res && fabs(d.res) <= 1.79e308)) { d.stop = true; d.status = MGCG_NONFINITE; }
    return d;
}
// Single-workgroup kernels that turn partial sums into the loop's scalars.
void launch_reduce_to(hipStream_t s, const double* partials, int n, double* dst, const int* done);          // dst = sum
void launch_reduce2_to(hipStream_t s, const double* pA, int nA, double* dstA, const double* pB, int nB, double* dstB, const int* done);   // two sums, one launch
void launch_finalize(hipStream_t s, const double* partials, const double* partialsInf, int n, bool reduceFirst, const FinalizeArgs& f);
void launch_finalize_precond(hipStream_t s, const double* partials, int n, bool reduceFirst, CgScalars* sc);  // rzNew -> beta, rr
void launch_init_scalars(hipStream_t s, const double* partials, const double* partialsZ, int n, bool reduceFirst, CgScalars* sc, HostMirror* mirror);   // partialsZ: null, or r.z (Jacobi)

// ---------------------------------------------------------------- multigrid kernels
// dinvUniform: dinv[i] == dinvScalar for every i (the array is then not read)
void launch_jacobi_first(hipStream_t s, long long n, double omega, const double* dinv, int dinvUniform, double dinvScalar, const double* b, double* x, const int* done);
// *flag = 1 if some v[i] differs (bitwise) from v[0]; flag pre-set to 0 by the caller
void launch_uniform_check(hipStream_t s, const double* v, long long n, int* flag);
void launch_restrict(hipStream_t s, int nx, int ny, int nz, const double* r, double* bc, const int* done);
void launch_prolong_add(hipStream_t s, int nx, int ny, int nz, double* x, const double* e, const int* done);
// x[i] = outer * (inner * b[i]) + e[parent(i)]   (prolong_add onto a first Jacobi sweep that was never stored)
void launch_prolong_linear_add(hipStream_t s, int nx, int ny, int nz, int z0, int z1, double* x, const double* eFull, const int* done);
void launch_restrict_linear(hipStream_t s, int nx, int ny, int nz, int z0, int z1, const double* rFull, double* bc, const int* done);
void launch_prolong_scaled(hipStream_t s, int nx, int ny, int nz, double* x, const double* b, double inner, double outer, const double* e, const int* done);
void launch_extract_dinv(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces,
                         long long n, long long rowBase, double* dinv);
// Galerkin: count pass (elementsC == nullptr) writes per-row counts to countsC[I]; fill pass writes entries.
void launch_galerkin(hipStream_t s, int nx, int ny, int nz, int zBegin, int zEnd, const double* elements, const int* rowOffsets, const int* columnIndeces,
                     double sigma, const int* rowOffsetsC, int* countsC, double* elementsC, int* columnIndecesC, int* errFlag);
void launch_poisson(hipStream_t s, int nx, int ny, int nz, int zBegin, int zEnd, double* elements, int* rowOffsets, int* columnIndeces);
void launch_rebase(hipStream_t s, int* rowOffsets, long long n, int base);
long long poisson_nnz_host(int nx, int ny, int nz, int zBegin, int zEnd);
void launch_minmax_int(hipStream_t s, const int* v, long long n, int* out2 /* device int[2] */);
void launch_halo_rows(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, long long offset, int* out2 /* {0, n} */);

// ---------------------------------------------------------------- aggregation multigrid kernels (kernels_amg.hip)
// the cycle's indexed transfer: bc[I] = serial sum of r over members[aggOffsets[I] .. aggOffsets[I+1]) from +0.0; x[i] += e[agg[i]]
void launch_amg_restrict(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const double* r, double* bc, const int* done);
void launch_amg_prolong_add(hipStream_t s, long long n, const int* agg, double* x, const double* e, const int* done);
// *badRow (pre-set to INT_MAX) = the smallest row whose diagonal is not stored, not finite or not positive
void launch_amg_check_diagonal(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, int* badRow);
// one matching pass: the row maxima once, then rounds (pick + match; flags2 pre-set to {0, 0}: {some row picked, some pair formed}); match pre-set to -1
void launch_amg_row_max(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, double* rowMax);
void launch_amg_match_round(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, long long n, double theta,
                            const double* rowMax, int* match, int* pick, int* flags2);
// sigma * P^T A P for a map: count pass (unique coarse columns per row, left sorted in the row's scratch segment), then the fill pass
void launch_amg_galerkin_count(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                               const int* agg, const int* expandOffsets, int* scratch, int* counts);
void launch_amg_galerkin_fill(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const double* elements, const int* rowOffsets,
                              const int* columnIndeces, const int* agg, const int* expandOffsets, const int* scratch, const int* rowOffsetsC, double sigma,
                              double* elementsC, int* columnIndecesC);
// out[k] = elements[source[k]], k < m: the values of the merged matrix [A | A^T] of MgcgSymmetricPart through its source list
void launch_amg_gather_values(hipStream_t s, long long m, const int* source, const double* elements, double* out);

// ---------------------------------------------------------------- the numeric refresh of an aggregation hierarchy (kernels_refresh.hip; MgUpdateValues)
constexpr int kRefreshTile = 2048;         // entries of the source list a workgroup stages in LDS at a time (16 KiB of values)
// The source list of sigma * P^T A P, built once per level from the pattern and the map (C's offsets and columns as the set-up left them).
// Count pass: counts[q] (zeroed, nnz(C) + 1 ints) = the entries of A behind coarse entry q; the caller scans them into segment offsets.
// Fill pass: sources[segment of q] = the stored positions of those entries in the contract's order; cursor = a copy of the offsets (consumed).
void launch_refresh_sources_count(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                                  const int* agg, const int* rowOffsetsC, const int* columnIndecesC, int* counts);
void launch_refresh_sources_fill(hipStream_t s, long long nc, const int* aggOffsets, const int* members, const int* rowOffsets, const int* columnIndeces,
                                 const int* agg, const int* rowOffsetsC, const int* columnIndecesC, int* cursor, long long held, int* sources);
// elementsC[q] = sigma * (((+0.0 + a[src[o]]) + a[src[o + 1]]) + ...), o in [segmentOffsets[q], segmentOffsets[q + 1]), q < segments
void launch_refresh_numeric(hipStream_t s, long long segments, long long sourceCount, const int* segmentOffsets, const int* sources, const double* elements,
                            double sigma, double* elementsC);
void preload_kernels_refresh();

// ---------------------------------------------------------------- the K-cycle's vector passes (kernels_kcycle.hip; MgSetCycle)
// Vectors of n rows of one coarse level; `partials`: that level's kKcycleSums regions of kMaxGrid doubles (0 rho1, 1 beta1, 2 gamma, 3 beta,
// 4 a2).  inner 0: u = c, 1: u = v.  The sums passes return the partial sums per region (1 under dot_order = 1), which the next pass takes.
constexpr int kKcycleSums = 5;
int  launch_kcycle_sums1(hipStream_t s, int inner, const double* c1, const double* v1, const double* b, long long n, double* partials, const int* done);
int  launch_kcycle_sums2(hipStream_t s, int inner, const double* c2, const double* v2, const double* v1, const double* rr, long long n, double* partials, const int* done);
// rr = b - a1 v1 with a1 = beta1 / rho1, or b when rho1 broke down
void launch_kcycle_residual(hipStream_t s, const double* b, const double* v1, double* rr, long long n, const double* partials, int nPartials, const int* done);
// e = k1 c1 + k2 c2 (c1 / a1 c1 on a breakdown); e may be c2
void launch_kcycle_combine(hipStream_t s, const double* c1, const double* c2, double* e, long long n, const double* partials, int nPartials, const int* done);
void preload_kernels_kcycle();

// ---------------------------------------------------------------- CSR transposition (kernels_transpose.hip; MgcgCsrTranspose, MgcgSymmetricPart)
constexpr int kTransposeShortMax = 32;     // a column stored this often or less is sorted by one lane in registers
constexpr int kTransposeLdsMax = 4096;     // ... this often or less by one workgroup in LDS; a longer one by one workgroup in global memory
// status3[0] (pre-set to INT_MAX) = the smallest row whose offsets descend, status3[1] = rowOffsets[0], status3[2] = rowOffsets[rows]
void launch_transpose_check_offsets(hipStream_t s, const int* rowOffsets, long long rows, int* status3);
// counts[c] (zeroed) = how often column c is stored; *badRow (pre-set to INT_MAX) = the smallest row that stores a column outside [0, columns).
// The offsets must have passed the check above and end at nnz.
void launch_transpose_count(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long columns, long long nnz, int* counts, int* badRow);
// keys[offsetsT[c] .. offsetsT[c + 1]) = (k << 32) | row of the stored entries of column c by ascending stored position k; offsetsT = the
// scanned counts; scratch: cursor (columns ints), work (1 + min(columns, nnz / (kTransposeShortMax + 1)) ints)
bool launch_transpose_claim_and_sort(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long columns, long long nnz,
                                     const int* offsetsT, int* cursor, int* work, unsigned long long* keys);
// A^T's columns (the rows of A), source list and values from the keys; outSource and outElements (with elements) may be null
void launch_transpose_emit(hipStream_t s, long long nnz, const unsigned long long* keys, const double* elements, int* outColumns, int* outSource, double* outElements);
// the merged matrix [A | A^T] of a square matrix: offsets (n + 1), columns and source list (2 nnz each)
void launch_transpose_merged(hipStream_t s, const int* rowOffsets, const int* columnIndeces, const int* offsetsT, const unsigned long long* keys, long long n, long long nnz,
                             int* mergedOffsets, int* mergedColumns, int* mergedSource);
void preload_kernels_transpose();

// ---------------------------------------------------------------- CSR matrix product C = A B (kernels_multiply.hip; MgcgCsrMultiply)
constexpr int kMultiplyShortMax = 32;      // a row of C of this many products or fewer is formed by one lane in registers
constexpr int kMultiplyLdsMax = 2048;      // ... of this many or fewer by one workgroup in LDS; a longer one by one workgroup in global scratch
constexpr int kMultiplyLongGrid = 64;      // workgroups that walk the work list for such rows, at the most: each holds scratch for the longest row
struct MultiplyArgs {
    const double* elementsA; const int* rowOffsetsA; const int* columnIndecesA;      // elementsA, elementsB null: the pattern alone
    const double* elementsB; const int* rowOffsetsB; const int* columnIndecesB;
    long long rows;
    const int* products;                   // u_i, the products of row i of C (launch_multiply_products)
    const int* work;                       // work[0] rows above the register class, listed from work[1]
    int* lengths;                          // count pass: the stored entries of every row of C
    const int* offsetsC; int* outColumnIndeces; double* outElements;                 // fill pass (outElements null: the pattern alone)
    unsigned long long* scratchKeys; double* scratchProducts; long long scratchStride;
};
// *badRow (pre-set to INT_MAX) = the smallest row that stores a column outside [0, bound).  The offsets have passed their check and end at nnz.
void launch_multiply_check_columns(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long rows, long long bound, long long nnz, int* badRow);
// products[i] = u_i; stat2 (pre-set to {INT_MAX, 0}) = {the smallest row with more than INT_MAX products, the largest u_i above
// kMultiplyShortMax}; work (work[0] zeroed, rows + 1 ints) lists the rows above the register class
void launch_multiply_products(hipStream_t s, const int* rowOffsetsA, const int* columnIndecesA, const int* rowOffsetsB, long long rows, int* products, int* work, int* stat2);
// the count pass (fill false) or the fill pass over every row of C; listed = work[0], longest = stat2[1]
bool launch_multiply_pass(hipStream_t s, const MultiplyArgs& a, bool fill, int listed, int longest, int longGrid);
// *total (zeroed) = the sum of lengths[0 .. rows) in 64 bits
void launch_multiply_total(hipStream_t s, const int* lengths, long long rows, unsigned long long* total);
void preload_kernels_multiply();

// ---------------------------------------------------------------- multicolour Gauss-Seidel smoother (kernels_gs.hip; MgSetSmoother)
// one colouring round: colourIn (-1 = uncoloured) -> colourOut; flags[0] = 1 if a row is left uncoloured; *badRow (pre-set to INT_MAX) = the
// smallest row whose neighbours hold all 64 colours
void launch_gs_colour_round(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, const int* colourIn, int* colourOut, int* flags, int* badRow);
// *badRow (pre-set to INT_MAX) = the smallest row that stores an entry of another row of its own colour
void launch_gs_check(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, const int* colour, int* badRow);
void launch_gs_zero(hipStream_t s, long long n, double* x, const int* done);
// x_i += omega * (dinv_i * (b_i - sum_k a_ik x_col)) in place for the rows of one colour, every sum in stored order; avgRow (the level's
// entries per row) picks the lanes that share a row's loads
void launch_gs_sweep(hipStream_t s, const int* rows, int count, const double* elements, const int* rowOffsets, const int* columnIndeces,
                     const double* b, const double* dinv, double omega, double* x, double avgRow, const int* done);
void preload_kernels_gs();

// ---------------------------------------------------------------- multicolour ILU(0) (kernels_ilu.hip; MgSetupIlu0)
// `lanes`: the lanes that share a row (4, 8 or 16, picked from the matrix's entries per row as launch_gs_sweep picks them)
// flags3[0 .. 2] (pre-set to INT_MAX) = the smallest row that stores a column outside [0, n) / that is empty / that stores no diagonal
void launch_ilu_check_rows(hipStream_t s, const int* rowOffsets, const int* columnIndeces, long long n, int* flags3);
// lengths[i] = the length of old row rowOf[i], i < n; lengths[n] = 0 (n + 1 ints: exclusive_scan makes B's offsets of them)
void launch_ilu_lengths(hipStream_t s, const int* rowOffsets, const int* rowOf, long long n, int* lengths);
// B = P (A + shift diag(A)) P^T, every row sorted by new column; diagPos[i] = where row i's diagonal stands; *dupRow (pre-set to INT_MAX) =
// the smallest old row that stores a column twice.  The rows must have passed launch_ilu_check_rows.
void launch_ilu_build(hipStream_t s, const double* elements, const int* rowOffsets, const int* columnIndeces, const int* rowOf, const int* newOf, long long n,
                      double shift, const int* offsetsB, double* valuesB, int* columnsB, int* diagPos, int* dupRow, int lanes);
// the IKJ elimination in place of new rows [row0, row0 + count), one colour, and their pinv; *badRow (pre-set to INT_MAX) = the smallest old
// row of them whose pivot is zero or not finite
void launch_ilu_factor(hipStream_t s, int row0, int count, const int* offsetsB, const int* columnsB, const int* diagPos, double* valuesB, double* pinv,
                       const int* rowOf, int* badRow, int lanes);
// partials[2 b], partials[2 b + 1] = smallest and largest pivot seen by block b; returns the blocks (kMaxGrid at the most)
int launch_ilu_pivot_range(hipStream_t s, const double* valuesB, const int* diagPos, long long n, double* partials);
// one colour of the forward (y_i = r[rowOf[i]] - sum l_ik y_k) or backward (t_i = pinv_i (y_i - sum u_ij t_j), z[rowOf[i]] = t_i) pass
void launch_ilu_pass(hipStream_t s, bool backward, int row0, int count, const double* valuesB, const int* offsetsB, const int* columnsB, const int* diagPos,
                     const double* pinv, const int* rowOf, const double* r, double* y, double* t, double* z, int lanes, const int* done);
void preload_kernels_ilu();

// ---------------------------------------------------------------- RCCL (dlopen'ed)
struct CommImpl;
bool comm_allreduce_sum(MgcgComm* c, double* devPtr, int count, hipStream_t s);
bool comm_multi(const MgcgComm* c);   // several ranks, or one rank forced onto the several-ranks path (force_multirank knob)
struct HaloPlan;  // per-peer contiguous send/recv ranges of p
// columnIndeces / nnz (device; may be null): when the slice is unstructured (the contiguous ranges come to a quarter of the vector or
// more) the plan is rebuilt from the column ids actually referenced -- per-peer index lists, packed and unpacked around the exchange.
// reuse: the plan of a solve's own vector p -- kept on the communicator and handed out again while every rank calls with the same partition
// (one 8-byte all-reduce decides); such a plan is not freed by halo_plan_destroy.  Plans of multigrid levels are never shared.
HaloPlan* halo_plan_create(MgcgComm* c, long long count, long long offset, long long countLocal, int minJ, int maxJ,
                           const int* columnIndeces = nullptr, long long nnz = 0, bool reuse = false, bool localOk = true);
// localOk (reuse plans only, several ranks): this rank's verdict on its own arguments, folded into the plan's one all-reduce -- when any
// rank says false, every rank gets nullptr and nobody enters the solve's collectives.
bool comm_agree(MgcgComm* c, bool localOk, const char* who);
bool comm_all(MgcgComm* c, bool mine, bool* all);                 // do all ranks say yes?  (a "no" is not an error)
// set-up only (collective): host vectors to and from ranks rank - 1 and rank + 1
bool comm_neighbour_exchange_host(MgcgComm* c, const std::vector<double>& toLower, const std::vector<double>& toUpper,
                                  std::vector<double>& fromLower, std::vector<double>& fromUpper, bool localOk = true);   // the same agreement as a call of its own (set-up paths)
void halo_last(long long out[3]);   // calling thread's last exchange: {index lists used, entries received, entries the contiguous plan receives}
void halo_plan_destroy(HaloPlan* h);
bool halo_exchange(MgcgComm* c, HaloPlan* h, double* p, hipStream_t s);
// interior rows on a side stream while the halo travels on the main stream (all RCCL calls stay on the main stream)
bool halo_overlap_available(MgcgComm* c);
hipStream_t halo_overlap_fork(MgcgComm* c, hipStream_t mainStream);   // side stream, ordered after everything enqueued on mainStream so far
bool halo_overlap_join(MgcgComm* c, hipStream_t mainStream);          // mainStream waits for the side stream
// the measured overlap rule (collective; once per plan): *pays = this plan's exchange in line costs more than the hops that would hide it
bool halo_overlap_pays(MgcgComm* c, HaloPlan* h, double* vec, hipStream_t s, bool* pays);
void halo_overlap_clear_times();
void halo_overlap_last_times(double out[3]);   // calling thread's last decision: {measured?, exchange in line (us), fork + launch + join (us)}

} // namespace mgcg
