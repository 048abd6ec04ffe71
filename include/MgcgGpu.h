/*
 * MgcgGpu.h -- C ABI of libMgcgGpu.so, the MI355X (gfx950) replacement for the
 * reference's native library MgcgGpu.dll (the .cu files under Mgcg/cuBlas/MgcgGpu/), which the
 * C# solver classes bind with [DllImport(MgcgGpu.DLL_NAME, EntryPoint = "...")]
 * (Mgcg/cuBlas/Mgcg/MgcgGpu.cs:11).
 *
 * Part 1 declares the reference's 32 exports with identical names, argument
 * order and meaning (each cites the reference definition it replaces).  The
 * reference's `int&`/`double&` out-parameters are pointers here: identical at
 * the binary level on x86-64, which is what P/Invoke `out int` relies on.
 * `_stdcall` is a no-op on x64.
 *
 * Part 2 is additive (no reference analogue): error reporting, fused ops, the
 * device problem generator, the multigrid preconditioner and the
 * one-process-per-GPU RCCL solver.
 *
 * Conventions: plain pointers and sizes only; every function is safe to call
 * concurrently from different host threads working on different devices; the
 * current device is per host thread (SetDevice); every call is complete (its
 * results visible to the host / to later calls) when it returns a value, and
 * stream-ordered on the device's single stream otherwise (same contract as
 * cuBLAS/cuSPARSE on the default stream).  Errors never abort: the call
 * returns 0 / NaN / NULL, and MgcgGetLastError() holds a message.
 */
#ifndef MGCG_GPU_H
#define MGCG_GPU_H

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque handles.  In the reference these are heap pointers to the vendor
 * handles (cublasHandle_t*, cusparseHandle_t*, cusparseMatDescr_t*,
 * thrust::device_vector<T>*); here they are heap pointers to library-owned
 * structs.  Caller owns them and frees them with the matching Destroy/Delete. */
typedef struct MgcgBlas     MgcgBlas;      /* stream + reduction workspace           */
typedef struct MgcgSparse   MgcgSparse;    /* stream + SpMV launch state             */
typedef struct MgcgMatDescr MgcgMatDescr;  /* general matrix, index base 0           */
typedef struct Vector       Vector;        /* device double[]  (zero-initialised)    */
typedef struct VectorInt    VectorInt;     /* device int[]     (zero-initialised)    */

/* ===================================================================== */
/* Part 1: the reference's exports                                        */
/* ===================================================================== */

/* ---- Runtime.cu ---- */
int           GetDeviceCount(void);                                  /* Runtime.cu:7  */
void          SetDevice(int deviceID);                               /* Runtime.cu:15 */
MgcgBlas*     CreateBlas(void);                                      /* Runtime.cu:20 */
void          DestroyBlas(MgcgBlas* cublas);                         /* Runtime.cu:28 */
MgcgSparse*   CreateSparse(void);                                    /* Runtime.cu:34 */
void          DestroySparse(MgcgSparse* cusparse);                   /* Runtime.cu:42 */
MgcgMatDescr* CreateMatDescr(void);                                  /* Runtime.cu:48 */
void          DestroyMatDescr(MgcgMatDescr* matDescr);               /* Runtime.cu:58 */

/* ---- Vector_Double.cu ---- (counts and offsets in ELEMENTS) */
Vector* Create_Double(int size);                                                       /* :7  */
void    CopyToArray_Double(const Vector* source, double destination[],
                           int count, int sourceOffset, int destinationOffset);        /* :15 */
void    CopyFromArray_Double(Vector* destination, const double source[],
                             int count, int sourceOffset, int destinationOffset);      /* :22 */
void    Delete_Double(Vector* vec);                                                    /* :29 */
double* ToRawPtr_Double(Vector* vec);                                                  /* :35 */
/* Vector_Double.cu:41.  The reference passes `count` as the BYTE count to
 * cudaMemcpy (missing *sizeof(double)); here count is in elements, as the
 * name and every other export imply. */
void    CopyFromDevice_Double(const double* source, double* destination,
                              int count, int sourceOffset, int destinationOffset);

/* ---- Vector_Int.cu ---- */
VectorInt* Create_Int(int size);                                                       /* :9  */
void       CopyToArray_Int(const VectorInt* source, int destination[],
                           int count, int sourceOffset, int destinationOffset);        /* :17 */
void       CopyFromArray_Int(VectorInt* destination, int source[],
                             int count, int sourceOffset, int destinationOffset);      /* :24 */
void       Delete_Int(VectorInt* vec);                                                 /* :31 */
int*       ToRawPtr_Int(VectorInt* vec);                                               /* :37 */

/* ---- Mgcg.cu: ops on RAW DEVICE POINTERS ---- */
/* y = alpha*A*x + beta*y, A general CSR, 0-based int32 (Mgcg.cu:10-19, was cusparseDcsrmv_v2).
 * Columns may be unsorted within a row.  beta == 0 never reads y. */
void   CsrMV(MgcgSparse* cusparse, MgcgMatDescr* matDescr,
             double* y,
             const double* elements, const int* rowOffsets, const int* columnIndeces,
             const double* x,
             int elementsCount, int rowCount, int columnCount,
             double alpha, double beta);
void   Axpy(MgcgBlas* cublas, double* y, const double* x, int count, double alpha);    /* y += alpha x   Mgcg.cu:22 */
double Dot(MgcgBlas* cublas, double* y, const double* x, int count);                   /* sum x_i y_i    Mgcg.cu:30 */
void   Scal(MgcgBlas* cublas, double* x, double alpha, int count);                     /* x *= alpha     Mgcg.cu:41 */
void   Copy(MgcgBlas* cublas, double* y, const double* x,
            int count, int yOffset, int xOffset);                                      /* y[yOff..] = x[xOff..]  Mgcg.cu:49 */

/* ---- Mgcg.cu: multi-device partition set-up and halo staging (HOST arrays in) ---- */
/* Mgcg.cu:57-85: upload rows [offsetForDevice, +countForDevice) of A, rebase the
 * row offsets by elementOffsetForDevice, upload the x and b slices, seed
 * p[offsetForDevice..] = x slice, return min/max column id of the slice. */
void Initialize(const double elements[], const int rowOffsets[], const int columnIndeces[],
                const double x[], const double b[],
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector,
                Vector* pVector,
                int* minJ, int* maxJ,
                int count,
                int countForDevice, int offsetForDevice, int elementCountForDevice, int elementOffsetForDevice);
/* Mgcg.cu:88-99: publish the first lastCount and last nextCount entries of this
 * device's slice of p into the shared host array p[]. */
void P2Host(Vector* pVector, double p[], int thisCount, int thisOffset, int lastCount, int nextCount);
/* Mgcg.cu:102-113: pull the lastCount entries before and nextCount entries after
 * this device's slice from the shared host array into pVector. */
void P2Device(Vector* pVector, double p[], int thisCount, int thisOffset, int lastCount, int nextCount);

/* ---- Mgcg.cu: the CG loop split at its three global-scalar dependencies ---- */
/* Mgcg.cu:116-142: Ap = A_loc p; r = b - Ap; p[offset..] = r; returns r.r (local) */
double Solve0(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
              Vector* xVector, Vector* bVector,
              Vector* ApVector, Vector* pVector, Vector* rVector,
              int count,
              int countForDevice, int offsetForDevice, int elementsCountForDevice);
/* Mgcg.cu:145-163: Ap = A_loc p; returns p_loc.Ap (local) */
double Solve1(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
              Vector* ApVector, Vector* pVector,
              int count,
              int countForDevice, int offsetForDevice, int elementsCountForDevice);
/* Mgcg.cu:166-184: x += alpha p_loc; r -= alpha Ap; returns r.r (local) */
double Solve2(MgcgBlas* cublas, double alpha,
              Vector* xVector,
              Vector* ApVector, Vector* pVector, Vector* rVector,
              int countForDevice, int offsetForDevice);
/* Mgcg.cu:187-198: p_loc = beta p_loc + r */
void   Solve3(MgcgBlas* cublas, double beta,
              Vector* pVector, Vector* rVector,
              int countForDevice, int offsetForDevice);

/* Mgcg.cu:201-270: the whole single-device CG.  x is initial guess and result.
 * *iteration = number of loop bodies executed (last index + 1, as the
 * reference's post-incremented counter); *residual = sqrt(r.r) of the
 * recurrence residual.  Stop rule (minIteration <= it) && (residual <
 * allowableResidual).  Unlike the reference (which never reads maxIteration and
 * spins forever on NaN), the loop also ends after index maxIteration or on a
 * non-finite residual; MgcgGetLastError() then says so. */
void Solve(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
           Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
           Vector* xVector, Vector* bVector,
           Vector* ApVector, Vector* pVector, Vector* rVector,
           int elementsCount, int count,
           double allowableResidual, int minIteration, int maxIteration,
           int* iteration, double* residual);

/* ===================================================================== */
/* Part 2: additive exports (no reference analogue)                       */
/* ===================================================================== */

/* Thread-local message of the last failed call ("" if none); cleared by MgcgClearLastError. */
const char* MgcgGetLastError(void);
void        MgcgClearLastError(void);
/* Library ABI revision (3 since round 5: exports added, Vector grew, 14 tuning knobs retired, dot_order added). */
int         MgcgAbiVersion(void);
/* Tuning knobs (15).  Every MGCG_* environment variable the library honours is read once, at first use; launches never read the
 * environment.  No knob changes an element-wise result (SpMV rows, vector updates, the V-cycle: the same doubles under every
 * setting).  What a SCHEDULE knob may change is how a dot product's partial sums are grouped: "overlap" reduces p.Ap from the
 * interior rows' launch and the boundary rows' launch instead of one launch, so with the default overlap = 1 -- a decision taken
 * from a timing -- two runs of a several-ranks solve on >= 1 M rows per rank can differ in the last bits of alpha / beta (1e-16
 * relative; near the tolerance, by one iteration).  For reproducible bits set overlap to 0 or 2, or dot_order to 1 (which makes
 * every sum independent of every schedule).  bench.py's N > 1 line names the schedule that ran.
 *   overlap (MGCG_OVERLAP: 0 halo exchange in line; 1 [default] hidden behind the interior rows where that pays BY MEASUREMENT -- for
 *     slices of >= 1 M rows per rank the plan's own exchange is timed in line against the fork / launch / join round trip of the overlap
 *     schedule on the live communicator, once per plan, and every rank takes the same decision from the all-reduced times; 2 whenever an
 *     interior exists);
 *   halo_stream (overlap schedule: 0 [default] the interior rows run on the communicator's side stream and every RCCL call on the
 *     main stream; 1 the halo exchange runs on the side stream and all rows on the main stream -- opt-in until RCCL on two streams of
 *     one communicator has been run on real multi-GPU hardware);
 *   deep_halo (MGCG_DEEP_HALO, default 1: the row-partitioned V(1,1) cycle takes ONE exchange per level -- a few planes of the level's
 *     right-hand side, after which everything within reach of the slab's boundaries is recomputed locally, bit for bit what the owner
 *     computes -- 4 exchanges per MGCG iteration; 0: one exchange per SpMV-shaped pass, 8 per iteration.  Needs slabs at least as thick
 *     as the halo on every coarse level (2 planes; nu_c on the coarsest), else the library takes the per-pass schedule by itself);
 *   no_fold (MGCG_NO_FOLD: the first Jacobi sweep of a V(1,.) cycle is stored instead of being formed per gather of the residual pass);
 *   fold_up (MGCG_FOLD_UP: -1 [default] the prolongation of a V(1,1) cycle is formed per gather of the post-smoothing sweep on levels of
 *     up to 100 M rows, 0 never, 1 on every level);
 *   check_every (iterations enqueued ahead of the stop flag, default 4);
 *   auto_tiles (MGCG_AUTO_TILES, default 1: Solve-family and per-op calls build column tiles themselves for matrices without locality);
 *   tile_shift (MGCG_TILE_SHIFT: column tiles of 2^shift columns; 0 [default] equal-width tiles of about 2.85 MiB of x),
 *     tile_pack (MGCG_TILE_PACK, default 1: 12-byte tile entries; 0 the 16-byte form);
 *   placement (MGCG_PLACEMENT, default 3: the first CG Solve-family call on vectors of >= 32 M entries times the loop's SpMV on that many
 *     EXTRA allocations of Ap, keeps the fastest, and then does the same for p -- where the runtime places the two vectors moves the
 *     SpMV by up to 17 %, the written one most; 0: off; a vector whose address ToRawPtr_Double has handed out is never moved; the
 *     preconditioned loop draws only when maxIteration leaves room to win the draw's cost back);
 *   dot_order (MGCG_DOT_ORDER, default 0; VALIDATION ONLY: 1 = every dot product adds its rounded products strictly left to right, the
 *     ranks' sums are added in rank order and SpMV rows are always summed in stored order -- the reference CPU twin's arithmetic,
 *     LongVector.cs:15-31, SparseMatrix.cs:68-88, resultsDot.Sum() -- so residual traces and iterates EQUAL the oracle's bit for bit at
 *     every size and rank count; one serial sum of 1.3e8 terms takes ~0.5 s: never on a timed path);
 *   verbose (MGCG_VERBOSE: errors and decisions also go to stderr);
 *   virtual_devices (MGCG_VIRTUAL_DEVICES: one physical GPU shown as n devices, tests only);
 *   force_multirank (MGCG_FORCE_MULTIRANK = w > 0: a one-rank RCCL communicator takes the several-ranks code path with an
 *     artificial halo of w entries, for measuring that path's device-side cost on a one-GPU box);
 *   fail_comm_init (MGCG_FAIL_COMM_INIT, tests only: MgcgCommInitAll / MgcgCommInitRank report failure, as on a host whose RCCL
 *     cannot form a communicator -- callers must then fall back or fail loudly).
 * (MGCG_COMPRESSION and the MGCG_SPMV_* variables are per-handle defaults of MgcgSetMatrixCompression / MgcgSetSpmv*, read by
 * CreateSparse.)  Knobs whose A/B was settled in rounds 2-4 have been removed with their settled value compiled in.
 * Loop-shape knob (1), beside the list above:
 *   x_defer (MGCG_X_DEFER, default 8, at most 8; 1 = one x update per iteration): the one-rank unpreconditioned loop keeps the
 *     directions of a group of this many iterations in a ring (the caller's p and x_defer - 1 library-owned vectors of the same size,
 *     held by the MgcgBlas handle) and applies x += alpha p for the whole group, oldest first, in the group's last iteration -- the same
 *     rounded operations as one term per iteration, so x, r, p and Ap are the same bits after every call.  A solve that stops inside a
 *     group applies its terms in the stopping iteration.  Several ranks and MGCG keep one term per iteration; if the ring cannot be
 *     allocated (2 GiB of HBM are always left free) the loop takes x_defer = 1 by itself (MGCG_VERBOSE=2 says so).
 * MgcgSetTuning / MgcgGetTuning take the knob's name or its environment variable; they return 0, or -1 for an unknown
 * name (MgcgGetLastError).  MgcgReloadEnvironment reads all variables again.  Change knobs only while no solve is running. */
int         MgcgSetTuning(const char* name, int value);
int         MgcgGetTuning(const char* name, int* value);
void        MgcgReloadEnvironment(void);
/* Wait for the current device's stream.  Returns 0 on success. */
int         MgcgDeviceSynchronize(void);
/* Elapsed-time helpers on the current device's stream (HIP events). */
void*       MgcgEventCreate(void);
void        MgcgEventRecord(void* ev);
float       MgcgEventElapsedMs(void* start, void* stop);   /* synchronises on stop */
void        MgcgEventDestroy(void* ev);
/* Free / total bytes of HBM on the current device. */
int         MgcgMemGetInfo(long long* freeBytes, long long* totalBytes);
/* 64-bit-size vector creation (Create_Double takes int). */
Vector*     MgcgCreateDouble64(long long size);
VectorInt*  MgcgCreateInt64(long long size);
long long   MgcgVectorSize(const Vector* v);

/* ---- extra BLAS-1 / fused ops on raw device pointers ---- */
/* y = x + beta*y  (the reference's Scal+Axpy pair Mgcg.cu:197,265 in one pass) */
void   Xpay(MgcgBlas* cublas, double* y, const double* x, int count, double beta);
/* max_i |x_i|  (HandmadeCL residual norm, Mgcg/HandmadeCL/MgcgCL/Mgcg.cl:110-159) */
double NrmInf(MgcgBlas* cublas, const double* x, int count);
/* y = A x and returns sum_i w_i y_i in the same pass (w = the rows' own slice of x in CG) */
double CsrMVDot(MgcgBlas* cublas, MgcgSparse* cusparse,
                double* y, const double* elements, const int* rowOffsets, const int* columnIndeces,
                const double* x, const double* w,
                int elementsCount, int rowCount, int columnCount);
/* One fused pass of the kind the solvers run: the product A x with one of the six solver-only epilogues, on raw device pointers,
 * by the route the solvers take -- the handle's kernel id, tuning, period and matrix form (MgcgSetSpmvKernel, MgcgSetSpmvTuning,
 * MgcgSetSpmvPeriod, MgcgSetMatrixCompression) apply as they do to CsrMV.  acc_i is row i's sum in the order of the kernel or form
 * that serves the product (MgcgSetSpmvKernel); every product and sum below is rounded on its own, in the order written:
 *   MGCG_EPI_RESIDUAL       y_i = b_i - acc_i
 *   MGCG_EPI_RESIDUAL_DOT   the same, and the call returns sum_i y_i * y_i
 *   MGCG_EPI_JACOBI         y_i = xo_i + omega * (dinv_i * (b_i - acc_i))
 *   MGCG_EPI_JACOBI_DOT     the same, and the call returns sum_i b_i * y_i
 *   MGCG_EPI_CHEBYSHEV      d_i = c1 * d_i + c2 * (dinv_i * (b_i - acc_i)) ; y_i = xo_i + d_i   (d is read and rewritten)
 *   MGCG_EPI_CHEBYSHEV_DOT  the same, and the call returns sum_i b_i * y_i
 * dinv == NULL: every dinv_i is dinvScalar and no array is read.  xOuter != 0 (MGCG_EPI_RESIDUAL only): the multiplied vector is
 * xOuter * (xInner * x[col]), formed per gather -- served by the row-tile kernel (10) and by the row-pattern form (class 3) alone.
 * Rows: rowEnd == 0 and gapEnd == 0, the whole matrix; rowEnd > 0, rows [rowBegin, rowEnd) only; gapEnd > 0, every row but those
 * of [gapBegin, gapEnd) -- one launch of the row-tile kernel when both cuts are multiples of 256, two launches otherwise.  Rows
 * outside the selection are not written, and the returned sum runs over the selected rows.  The arrays always describe the whole
 * matrix: y, b, xo, dinv and d are indexed by row, x by column.  The Chebyshev epilogues multiply through the plain CSR kernels
 * whatever form the handle holds, and take whole matrices only.
 * done (may be NULL): a device int; when it is nonzero the pass writes nothing (and the returned value means nothing).
 * The returned sum (0.0 for the epilogues without one) is added up per workgroup and then over the workgroups, each in a fixed
 * order; under the knob dot_order = 1 it is formed again as CsrMVDot forms its own: one serial sum, left to right, over the selected
 * rows -- with a gap, the serial sum of the rows in front of the gap plus the serial sum of those behind it.
 * Refused (MgcgGetLastError, NaN returned, nothing launched): an epilogue outside the six; a null operand the epilogue reads; a
 * row range or gap outside the matrix, both at once, or either with a Chebyshev epilogue; xOuter != 0 with another epilogue
 * than MGCG_EPI_RESIDUAL, or where neither the row-tile kernel nor the row-pattern form serves the matrix; y overlapping b, xo,
 * x or d (the column-tiled and propagation-blocking forms accumulate in y). */
#define MGCG_EPI_RESIDUAL      2
#define MGCG_EPI_JACOBI        3
#define MGCG_EPI_RESIDUAL_DOT  4
#define MGCG_EPI_JACOBI_DOT    6
#define MGCG_EPI_CHEBYSHEV     7
#define MGCG_EPI_CHEBYSHEV_DOT 8
typedef struct MgcgEpilogueArgs {
    int epilogue;                 /* MGCG_EPI_* */
    int elementsCount, rowCount, columnCount;
    double* y;
    const double* elements; const int* rowOffsets; const int* columnIndeces;
    const double* x;
    const double* b;
    const double* xo;
    const double* dinv; double dinvScalar;
    double omega;
    double* d; double c1, c2;
    double xInner, xOuter;
    int rowBegin, rowEnd;
    int gapBegin, gapEnd;
    const int* done;
} MgcgEpilogueArgs;
double MgcgCsrMVEpilogue(MgcgBlas* cublas, MgcgSparse* cusparse, const MgcgEpilogueArgs* args);
/* SpMV kernel selection for CsrMV-family calls on this handle:
 * 0 auto, 1 row-block LDS stream kernel, 2..8 = 2^(k-2) lanes per row (k=2: one lane per row, the stored-order sum; k=8: one
 * wavefront per row), 9 row-block "stage raw, multiply by row" kernel, 10 row-tile kernel (256 rows per tile; the auto choice for
 * short rows).  9 and 10 need elementsCount >= 8 and 16-byte aligned elements, 10 also 16-byte and 9 8-byte aligned
 * columnIndeces; products that do not qualify fall back 10 -> 9 -> 1.  Kernels 1, 2, 9 and 10 add a row's rounded products in stored order; 3..8 let lane l add entries l, l + L, ... in
 * stored order and join the L sums in the tree acc_l += acc_(l + off), off = L/2 .. 1.  Every other value (negative, 11, ...) is
 * not an error: it runs what 8 runs.  A usable form of MgcgSetMatrixCompression takes precedence over this choice. */
void   MgcgSetSpmvKernel(MgcgSparse* cusparse, int kernel);
/* Tuning knobs of the stream kernel: rowsPerBlock in {64,128,256}, flags bit0 = non-temporal matrix
 * loads, bit1 = XCD-contiguous row-block mapping, bit2 = banded schedule; gridBlocks (0 = chip-filling default). */
void   MgcgSetSpmvTuning(MgcgSparse* cusparse, int rowsPerBlock, int flags, int gridBlocks);
/* Banded schedule hint for the stream kernel: periodRows = distance (in rows) of the far band of the
 * matrix, e.g. nx*ny for a 3-D stencil (sets flag bit2).  The Solve-family exports detect it themselves;
 * 0 switches the schedule off.  A period the kernel cannot use (not a multiple of 8 row blocks, not
 * tiling the matrix) silently falls back to the plain schedule.  Results are identical either way. */
void   MgcgSetSpmvPeriod(MgcgSparse* cusparse, int periodRows);
/* Tile of the banded schedule: tileRows neighbouring rows x tilePlanes consecutive windows are in flight
 * per XCD at a time (0, 0 = the library's default).  Pure scheduling: results do not change. */
void   MgcgSetSpmvTile(MgcgSparse* cusparse, int tileRows, int tilePlanes);

/* Opt-in analysis (the role cuSPARSE's csrmv analysis plays in the reference's stack): with compression enabled the
 * Solve-family, MgSetup and CsrMV/CsrMVDot on this handle re-encode a matrix ONCE into a lossless compact form and use
 * it for every later SpMV on the same arrays.  Results are bit-identical to the CSR kernels (same doubles, same order).
 *   enable = 1: the best form the matrix admits --
 *       class 3  one byte per ROW when the matrix has <= 256 distinct rows read as sequences of (col-row, value)
 *                pairs (constant-coefficient stencils: 27 for the 7-point Laplacian on a box; every Galerkin level),
 *       class 2  two bytes per nonzero when it has <= 256 distinct offsets col-row and <= 256 distinct values,
 *       class 1  one byte per nonzero + the fp64 value when only the offsets qualify,
 *       class 4  a column-tiled copy (16 bytes per nonzero MORE, not fewer) for sorted rows whose entries are spread over
 *                an x far larger than the L2: the gathers of a pass stay inside one 4 MiB window of x,
 *       class 0  otherwise (plain CSR kernels);
 *   enable = 3: the same choice as 1, but for a matrix without locality the propagation-blocking form comes before the column tiles
 *   (order 3, 2 / 1, 5, 4, 0) --
 *       class 5  x gathered from LDS in tiles of 16384 columns (pass 1 stores every product, pass 2 sums each block of 1024 rows in
 *                rounds of 9088 entries in stored order and applies the epilogue, beta != 0 included); about 20 bytes per nonzero MORE
 *                (10 B of entries, 8 B of products, 2 B of positions) plus 12 B per (row block, tile) and 2 KB per (block, round).
 *                Taken only for rows whose column tiles never step back (sorted rows suffice), a sampled mean distance from the
 *                diagonal of at least one tile, 2 .. 1024 tiles (x of at most 16.7 M columns), nnz < 2^31 and at most half of
 *                the free device memory; otherwise mode 3 falls through to class 4 and class 0 as mode 1 does (MGCG_VERBOSE=1
 *                prints why).  Whole products only: row ranges and multigrid levels use the other forms;
 *   enable = 2: per-nonzero codes only (classes 2 / 1 / 0);   enable = 0: off;   enable >= 4 means 1.
 * The cache is keyed by the array pointers and sizes: a caller that rewrites a matrix in place must call
 * MgcgAnalysisClear.  MgcgAnalysisInfo(index) reports a cached analysis: returns the class (-1 past the end);
 * distinctOffsets / distinctValues receive, for class 3, the number of distinct rows and the longest row; for class 4
 * the number of column tiles and 0; for class 5 the number of column tiles and the most rounds any row block takes. */
void   MgcgSetMatrixCompression(MgcgSparse* cusparse, int enable);
void   MgcgAnalysisClear(MgcgSparse* cusparse);
int    MgcgAnalysisInfo(MgcgSparse* cusparse, int index, int* distinctOffsets, int* distinctValues, long long* rows, long long* nnz);

/* Per-launch HIP-event timing of the SpMV kernel inside the Solve.. / CgSteps calls on this handle's stream:
 * enable, run, then read the summed milliseconds and the number of launches timed. */
void   MgcgProfileSpmv(MgcgSparse* cusparse, int enable);
double MgcgProfileSpmvMs(MgcgSparse* cusparse, int* launches);

/* ---- synthetic structured problems generated directly in HBM ---- */
/* nnz of rows z in [zBegin, zEnd) of the 5/7-point Poisson matrix on nx*ny*nz. */
long long MgcgPoissonNnz(int nx, int ny, int nz, int zBegin, int zEnd);
/* Fill the CSR slice for rows with z in [zBegin, zEnd): diagonal 2*dim, off-diagonals -1,
 * Dirichlet, lexicographic x-fastest, ascending GLOBAL column ids, row offsets rebased to the
 * slice (as Initialize does).  Vectors must hold MgcgPoissonNnz / rows+1 entries.  Returns 0 on success. */
int MgcgGeneratePoisson(Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        int nx, int ny, int nz, int zBegin, int zEnd);
/* min / max column id over the first elementCount entries (what Initialize returns as minJ, maxJ;
 * Mgcg.cu:83-84) for matrices that were generated on the device.  Returns 0 on success. */
int MgcgMinMaxColumn(VectorInt* columnIndecesVector, int elementCount, int* minJ, int* maxJ);
/* Fill a device vector with a constant. */
void MgcgFill(Vector* v, double value);

/* ---- solver with selectable stop rule ---- */
enum {
    MGCG_RULE_NATIVE     = 0,  /* Mgcg.cu:251-252   (min <= it) && res < tol                      */
    MGCG_RULE_CSHARP     = 1,  /* ConjugateGradient.cs:56-79  it<min: no; it>max: error; res<tol  */
    MGCG_RULE_SIMPLE     = 2,  /* SimpleConjugateGradient.cu:53,107  x:=0; (min < it) && res<tol  */
    MGCG_RULE_HANDMADECL = 3,  /* HandmadeCL ConjugateGradientCpu.cs:68-95  max-norm, C# rule     */
    MGCG_RULE_VIENNACL   = 4   /* ViennaCL ComputerGpu.cpp:78  (min < it) && rrNew/rr0 < tol^2    */
};
enum { MGCG_OK = 0, MGCG_MAXIT_EXCEEDED = 1, MGCG_NONFINITE = 3, MGCG_ERROR = -1 };
/* As Solve, plus: rule (above); residualTrace (host, may be NULL) receives the residual of each
 * iteration up to traceCapacity; returns a status code.  *iteration is the zero-based index of the
 * last executed loop body (what the C# classes expose as Iteration). */
int SolveEx(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
            Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
            Vector* xVector, Vector* bVector,
            Vector* ApVector, Vector* pVector, Vector* rVector,
            int elementsCount, int count,
            double allowableResidual, int minIteration, int maxIteration, int rule,
            int* iteration, double* residual,
            double* residualTrace, int traceCapacity);

/* ---- block CG: k right-hand sides per matrix pass (one rank, no preconditioner, plain CSR) ---- */
/* k (1..8) independent CG solves on one matrix, each iteration reading the matrix once for all k.  Column j of x, b and r lies at
 * [j*count, (j+1)*count) of its vector (k*count entries each); Ap and p are k*count entries of work space whose layout is internal
 * (row-interleaved).  Per column: the stop rule `rule` of SolveEx, its own iteration / residual / status (iteration[], residual[],
 * status[]: k entries each, may be NULL); a column that has stopped is not changed by later iterations.  residualTrace (may be
 * NULL): column j's trace at j*traceCapacity.  Every column is exactly the classical CG of SolveEx on that column (the k recurrences
 * share the matrix pass only); under dot_order = 1 its trace, iterate, residual and iteration equal SolveEx's / the oracle's bit for
 * bit.  The matrix is always read as plain CSR, whatever the handle's compression mode; placement draw and x_defer do not apply.
 * Returns MGCG_ERROR on a library error (k outside 1..8, a null handle, a vector that is too small; MgcgGetLastError), else the
 * worst column status (MGCG_NONFINITE > MGCG_MAXIT_EXCEEDED > MGCG_OK). */
int SolveBlockEx(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                 int elementsCount, int count, int k,
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int iteration[], double residual[], int status[], double residualTrace[], int traceCapacity);
/* y = A x for k (1..8) columns of a square count x count CSR matrix on raw device pointers, column j of x and y at [j*count, (j+1)*count),
 * the matrix read once.  Every row adds its rounded products in stored order: column j equals the stored-order product of column j alone
 * (CsrMV with alpha 1, beta 0 under dot_order = 1, or by its lane = row kernels), bit for bit.  Plain CSR, whatever the handle's
 * compression mode.  Stream-ordered; errors: MgcgGetLastError. */
void CsrMVBlock(MgcgSparse* cusparse, MgcgMatDescr* matDescr, double* y, const double* elements, const int* rowOffsets,
                const int* columnIndeces, const double* x, int elementsCount, int count, int k);

/* ---- multigrid preconditioner (defined by this build; the reference's "Mgcg" never implemented it) ---- */
typedef struct MgcgMg MgcgMg;
/* Geometric cell-centred hierarchy on an nx*ny*nz lexicographic grid for the CSR matrix in the
 * vectors (count = nx*ny*nz rows): piecewise-constant P, R = P^T, A_c = sigma*P^T A P, weighted-Jacobi
 * V(nu,nu), nuCoarse sweeps on the last level.  levels is clipped to what the grid allows. */
MgcgMg* MgSetup(MgcgBlas* cublas, MgcgSparse* cusparse,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                int elementsCount, int nx, int ny, int nz,
                int levels, double omega, int nu, int nuCoarse, double sigma);
/* The same on this rank's z-slab [zBegin, zEnd) of the grid (equal slabs in rank order; the vectors hold the local
 * rows with global column ids, as Initialize lays them out).  Every level keeps the slab aligned; per-level halo
 * planes travel over `comm` before each smoothing / residual pass.  comm == NULL: one rank. */
typedef struct MgcgComm MgcgComm;
MgcgMg* MgSetupParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        int elementsCount, int nx, int ny, int nz, int zBegin, int zEnd,
                        int levels, double omega, int nu, int nuCoarse, double sigma);
/* Aggregation multigrid: the same hierarchy -- piecewise-constant P, R = P^T, A_c = sigma*P^T A P, weighted-Jacobi V(nu,nu), nuCoarse
 * sweeps on the last level -- for ANY CSR matrix with a positive stored diagonal: the aggregates come from the matrix graph instead of
 * 2x2x2 boxes of a grid.  One rank.  MgApply, SolveMg, MgLevels, MgLevelRows, MgLevelNnz, MgLevelCopyCsr, MgLevelCopyDinv and MgDestroy
 * work on the result; MgSetInterpolation(mg, 1) returns -1 (the linear transfer needs a grid) and SolveMgParallel on a communicator of
 * several ranks refuses it.  The set-up is deterministic and defined by the data alone:
 *
 * One MATCHING PASS on a matrix B of n rows (assumed symmetric; not checked):
 *   1. a stored entry k of row i with column j != i and value < 0 couples i and j with weight w = -value; entries >= 0 and the diagonal
 *      do not couple.
 *   2. m_i = the largest w of row i, 0 if there is none.
 *   3. row i holds the candidate edge {i, j} iff w >= theta*m_i and w >= theta*m_j (w from row i).
 *   4. the tie-break key of an edge, 32-bit unsigned arithmetic, lo = min(i, j), hi = max(i, j):
 *        h = lo*0x9E3779B1 + hi*0x85EBCA77; h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15
 *   5. a round: every unmatched row picks the neighbour with the lexicographically largest (w, h, j) among those of its candidate edges
 *      whose other end is unmatched; rows that pick each other are matched.  Rounds repeat until no row has such an edge left (or, on an
 *      unsymmetric matrix, until a round matches nobody).  The host reads one flag pair per round.
 *   6. unmatched rows become singletons; aggregates are numbered by their smallest member, ascending.
 * One LEVEL takes `passes` (1..4; 3 gives aggregates of up to 8 rows, the size of the 2x2x2 box) matching passes: pass 1 on the level's
 * matrix, pass p > 1 on the unscaled Galerkin matrix (sigma = 1) of pass p - 1 (skipped once a pass matches nothing); the level's map is
 * their composition.  The next level's matrix is sigma*P^T A P of the level's own matrix with the composed map.
 * GALERKIN CONTRACT: coarse row I takes its members in ascending fine index and each member's entries in stored order; every value is
 * added to the accumulator of its coarse column, starting from +0.0; columns are emitted in ascending order, each as sigma*acc.  (The
 * order of MgSetup's Galerkin pass: box aggregates reproduce MgSetup's hierarchy and its V-cycle bit for bit.)  No matrix value travels
 * to the host; index bookkeeping (scans, the counting sort of a map into member lists) runs there.
 * The hierarchy ENDS with level l when `levels` is reached, when level l has <= minCoarse rows, or when the next level would keep more
 * than 3/4 of level l's rows ("nothing matched" included: a matrix without a negative off-diagonal entry gives ONE level, whose cycle is
 * nuCoarse Jacobi sweeps).  Every level's diagonal must be stored, finite and > 0: else NULL, the error names the level and the row.
 * In the cycle a level with a map runs the stored path: nu sweeps, r = b - A x, b_c[I] = the serial sum of r over I's members in ascending
 * order from +0.0, the next level, x[i] += e[agg[i]], nu sweeps.
 * Set-up (maps, level matrices, D^-1) is the same bits in every mode.  In the sweeps and the residual pass a level whose rows hold 20 entries
 * or fewer on average sums every row in stored order; longer rows are summed by several lanes whose partial sums meet in a tree, or in stored
 * order under dot_order = 1 -- as everywhere in the library.  Under dot_order = 1 M^-1 r is one fixed sequence of IEEE operations.
 * omega is the caller's (one value for all levels, not range-checked): omega*lambda_max(D^-1 A) < 2 on every level is the caller's
 * condition for a symmetric POSITIVE DEFINITE preconditioner (6/7 and 4/5 are MgSetup's values for the 7- and 5-point stencils).
 * Returns NULL with MgcgGetLastError() on bad arguments (a null handle, levels < 1, passes outside 1..4, theta outside (0, 1], vectors
 * that are too small: refused before a device is asked for). */
MgcgMg* MgSetupAggregation(MgcgBlas* cublas, MgcgSparse* cusparse,
                           Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           int elementsCount, int count, int levels, int passes, double theta, int minCoarse,
                           double omega, int nu, int nuCoarse, double sigma);
/* S = (A + A^T) / 2 of a square count x count CSR matrix, formed on the device into the caller's vectors (device vectors of the library,
 * as the input).  Returns the number of stored entries of S; with all three output vectors NULL it returns that count and writes nothing.
 * CONTRACT (one fixed sequence of IEEE operations, the same in every mode, no atomics on values):
 *   pattern: row i of S stores every column j that row i of A stores or whose own row j stores column i; columns ascend, each appears
 *            once.  A pair whose sum is zero is KEPT as a stored 0.0 (an entry >= 0 never couples in the matching: zeros change no map).
 *   value:   acc = +0.0; the stored entries of column j in row i of A are added in stored order; then the stored entries of column i in
 *            row j of A in stored order; s_ij = 0.5 * acc.
 * Hence: the diagonal of a row that stores it once comes out exactly (0.5 * (a + a)); S is symmetric bit for bit when no row stores a
 * column twice (two addends: the sum commutes); a symmetric matrix with ascending unique columns gives itself, pattern and values.  Rows
 * may be unsorted, hold duplicates and be of any length.  The offsets and columns are checked and the entries are ordered by column on the
 * device (the transposition of MgcgCsrTranspose below, pattern and source list); no entry-sized array and no matrix value travels to the
 * host -- two flags, the end of the offsets and, on a refusal, the one offending row do -- and the values are gathered and summed on the
 * device.  S is built in storage of the library's own (about 2 x elementsCount values and 6 x elementsCount ints while it runs, the
 * transposition's share of it freed before the sums are formed, and 3 x count ints) and copied out at the end: on a refusal the output
 * vectors are untouched.
 * Returns -1 with MgcgGetLastError() on a refusal.  Refused before a device is asked for: a null handle (the three output vectors are
 * given together or not at all), count < 1, elementsCount < 0, 2 * elementsCount above INT_MAX, input vectors smaller than elementsCount
 * / count + 1, output vectors smaller than outCapacity / count + 1.  Refused once the arrays have been read: offsets that do not start
 * at 0, descend or end beyond elementsCount, a column outside [0, count), and an outCapacity below the count of S (the message states
 * the count; a capacity of 2 * elementsCount always suffices). */
long long MgcgSymmetricPart(MgcgBlas* cublas, MgcgSparse* cusparse,
                            Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                            int elementsCount, int count,
                            Vector* outElements, VectorInt* outRowOffsets, VectorInt* outColumnIndeces, int outCapacity);
/* A^T of a rows x columns CSR matrix, formed on the device into the caller's vectors (device vectors of the library, as the input).
 * elementsVector NULL asks for the pattern alone (outElements is then NULL too; the two are given together or not at all).  Returns
 * rowOffsets[rows], the stored entries of A^T.
 * CONTRACT (no arithmetic, no atomics on values; two calls give identical arrays):
 *   row c of A^T holds the stored entries of column c of A by ascending stored position k (k = the index into elementsVector /
 *   columnIndecesVector: it ascends with the row of A and, inside one row, with the stored order -- so duplicates keep their order);
 *   outSource[q] = k (outSource may be NULL); outColumnIndeces[q] = the row of A that stores k; outElements[q] = elements[k], a bit copy
 *   (a NaN's payload and -0.0 survive); outRowOffsets holds columns + 1 offsets from 0.
 * Rows of A may be unsorted, may be empty and may hold duplicates; the matrix may be rectangular; a column that nobody stores gives an
 * empty row; entries of the input vectors beyond rowOffsets[rows] are ignored, entries of the output vectors beyond the result are left
 * alone.  The call is synchronous.  While it runs it holds 2 x elementsCount + 2 x columns ints of device storage of its own, and one
 * more for every column stored more than 32 times.  How: integer counts per column and their scan give the offsets; every entry claims
 * a slot of its column's segment, and every segment is then sorted by k -- by one lane in registers up to *shortMax = 32 entries, by one
 * workgroup in LDS up to *ldsMax = 4096, by one workgroup in global memory beyond that (slow, and correct for a column that every row
 * stores); MgcgTransposeClassLimits reports the two boundaries.
 * Returns -1 with MgcgGetLastError() on a refusal.  Refused before a device is asked for: a null handle, elementsVector and outElements
 * not given together, rows < 1, columns < 1, elementsCount < 0, input vectors smaller than elementsCount / rows + 1, output vectors
 * smaller than elementsCount / columns + 1.  Refused once the arrays have been read, with the outputs untouched: offsets that do not
 * start at 0, descend ("row %lld: the row offsets descend": the smallest such row) or end beyond elementsCount, and a column outside
 * [0, columns) ("row %lld stores column %d, the matrix has %lld columns": the smallest such row, its first such entry; the host reads
 * that one row to name the column). */
long long MgcgCsrTranspose(MgcgBlas* cublas, MgcgSparse* cusparse,
                           Vector* elementsVector /* NULL: pattern only */, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           int elementsCount, int rows, int columns,
                           Vector* outElements /* NULL iff elementsVector is NULL */, VectorInt* outRowOffsets, VectorInt* outColumnIndeces,
                           VectorInt* outSource /* may be NULL */);
void      MgcgTransposeClassLimits(int* shortMax, int* ldsMax);           /* the longest column of the register class and of the LDS class (either may be NULL) */
/* C = A B of two CSR matrices, A rows x inner and B inner x columns, formed on the device into the caller's vectors (device vectors of the
 * library, as the inputs).  elementsA NULL asks for the pattern alone (elementsB and outElements are then NULL too).  Returns the stored
 * entries of C.  With all three output vectors NULL it returns that count and writes nothing: the symbolic phase alone.
 * CONTRACT (one fixed sequence of IEEE operations, the same in every mode and in every call; no atomics on values):
 *   products: row i of A, walked in stored order, gives stored entries p with column k_p.  Each p contributes the stored entries q of row
 *             k_p of B, in stored order.  This numbers the products of row i as t = 0, 1, 2, ...
 *   pattern:  row i of C stores column j exactly when some product of row i lands on j.  Columns ascend and each appears once.  A sum
 *             that comes out zero is KEPT as a stored 0.0.
 *   value:    acc = +0.0; for the products that land on j, in ascending t: acc = acc + (a_p * b_q) -- the product is rounded, then the
 *             sum is rounded (no fused multiply-add) -- c_ij = acc.
 * Inputs allowed: either matrix may be rectangular.  Rows may be unsorted, empty and hold duplicates, in A and in B alike; duplicates are
 * separate products, in stored order.  A row of B that no entry of A points to takes no part: its values and, in the product, its columns
 * are never read (the column check below covers every stored entry of B).  Entries beyond rowOffsets[last] are ignored.  Output entries
 * beyond the result are left alone.  Non-finite values follow IEEE (inf * 0 is NaN); a NaN's payload is not promised.  Hence a lone
 * product -0.0 gives +0.0 (0.0 + -0.0), and an integer-valued product whose partial sums stay below 2^53 is exact.
 * How: one integer pass gives u_i, the products of row i of C; a count pass gives the stored entries of every row, the library's scan the
 * offsets, and a fill pass writes columns and values -- the count of C is known before anything is written, and no array of all products
 * exists.  Rows of C fall into three classes: u_i <= *shortMax = 32, one lane with columns and products in registers; u_i <= *ldsMax =
 * 2048, one workgroup that expands the keys (j << 32) | t into LDS, sorts them and lets the lane at a run's first key sum the run in
 * ascending t; longer rows, one workgroup doing the same in global scratch of the library's own (slow, correct, no limit but INT_MAX
 * products a row and the memory: 16 bytes a product of the longest row for each of up to 64 workgroups, 1 GiB of keys at the most).
 * MgcgMultiplyClassLimits reports the two boundaries.  While it runs the call also holds 3 x rows ints.  The call is synchronous.
 * Returns -1 with MgcgGetLastError() on a refusal.  Refused before a device is asked for: a null handle; value vectors and outElements
 * not given together; the three outputs not all given or all NULL; rows, inner or columns < 1; a negative element count or capacity;
 * input vectors smaller than their counts / rows + 1 / inner + 1; output vectors smaller than outCapacity / rows + 1.  Refused once the
 * arrays have been read, with the outputs untouched: offsets of A or B that do not start at 0, descend or end beyond the count (the
 * transposition's messages after "MgcgCsrMultiply: A: " or "... B: "); a column of A outside [0, inner) or of B outside [0, columns)
 * ("MgcgCsrMultiply: A: row %lld stores column %d, the matrix has %lld columns": the smallest such row, its first such entry); a row of
 * C with more than INT_MAX products, or a C of more than INT_MAX entries; an outCapacity below the count of C (the message states the
 * count). */
long long MgcgCsrMultiply(MgcgBlas* cublas, MgcgSparse* cusparse,
                          Vector* elementsA /* NULL: pattern only */, VectorInt* rowOffsetsA, VectorInt* columnIndecesA, int elementsCountA,
                          Vector* elementsB /* NULL iff elementsA is NULL */, VectorInt* rowOffsetsB, VectorInt* columnIndecesB, int elementsCountB,
                          int rows, int inner, int columns,          /* A: rows x inner, B: inner x columns */
                          Vector* outElements, VectorInt* outRowOffsets, VectorInt* outColumnIndeces, int outCapacity);
void      MgcgMultiplyClassLimits(int* shortMax, int* ldsMax);            /* the most products of a row of the register class and of the LDS class (either may be NULL; needs no device) */
/* MgSetupAggregation with a choice of what the matching reads.  strength = 0: the level's own matrix -- MgSetupAggregation, which is this
 * call with 0, bit for bit.  strength = 1: the matching of every level l runs on S_l, the symmetric part (MgcgSymmetricPart's contract) of
 * the level's OWN matrix A_l: pass 1 on S_l, pass p > 1 on the unscaled Galerkin matrix of pass p - 1 built from S_l; S_l is then freed
 * and the next level is sigma*P^T A_l P of A_l itself with that map.  Nothing else changes: the matching rules, theta, the key, the
 * numbering, the diagonal checks, the three end rules, the cycle, MgSetSmoother.  Why: on A != A^T the matching reads w = -a_ij from row i
 * alone and pairs rows on MUTUAL picks; where the strong entry of row i points upstream and row j's entry back is weak or >= 0 (upwind and
 * strong central convection) nothing pairs and the hierarchy has ONE level.  S_l has the couplings of both rows in both rows.  On a
 * symmetric matrix with ascending unique columns S_l = A_l and both strengths build the same hierarchy.  M stays a fixed linear operator:
 * what SolveBicgstabMg, SolveGmresMg (right preconditioning) ask.  Other values of strength are refused before a device is asked for. */
MgcgMg* MgSetupAggregationEx(MgcgBlas* cublas, MgcgSparse* cusparse,
                             Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                             int elementsCount, int count, int levels, int passes, double theta, int minCoarse,
                             double omega, int nu, int nuCoarse, double sigma, int strength);
int     MgStrength(const MgcgMg* mg);                                     /* the strength the hierarchy was built with (0 for NULL, MgSetup, MgSetupAggregates) */
/* The same hierarchy from the caller's aggregates (host arrays): levelRows[0 .. levels-1] are the rows of every level (levelRows[0] =
 * count), aggregateOf holds the maps of levels 0 .. levels-2 one after the other (levelRows[l] ids in [0, levelRows[l+1]) each).  Exactly
 * `levels` levels are built.  An id out of range or an empty aggregate is refused (NULL, MgcgGetLastError()). */
MgcgMg* MgSetupAggregates(MgcgBlas* cublas, MgcgSparse* cusparse,
                          Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                          int elementsCount, int count, int levels, const int levelRows[], const int aggregateOf[],
                          double omega, int nu, int nuCoarse, double sigma);
/* aggregateOf[0 .. MgLevelRows(level)-1] = the map of `level` to the next one.  Returns 0; -1 with MgcgGetLastError() on a geometric
 * hierarchy (MgSetup / MgSetupParallel) or on the last level. */
int     MgLevelCopyAggregates(const MgcgMg* mg, int level, int aggregateOf[]);
void    MgDestroy(MgcgMg* mg);
/* Transfer operators of the V-cycle: 0 (default) piecewise-constant P, 1 cell-centred linear P (per coarsened dimension
 * a child takes 3/4 of its parent and 1/4 of the parent's neighbour on the child's side), R = P^T in both; the coarse
 * operators are the same.  With several ranks the call is collective (it plans one extra plane exchange per level and
 * transfer).  Returns 0, or -1 with MgcgGetLastError(). */
int     MgSetInterpolation(MgcgMg* mg, int mode);
/* The smoother of the V-cycle: 0 (default) weighted Jacobi, 1 multicolour Gauss-Seidel.  Mode 1 is for aggregation hierarchies
 * (MgSetupAggregation / MgSetupAggregates: one rank, every level stored; a geometric hierarchy is refused -- MgSetupAggregates with 2x2x2
 * box maps builds the same one) with an EVEN nuCoarse.  A Gauss-Seidel sweep on a symmetric positive definite matrix converges for every
 * 0 < omega < 2, and the cycle below is a symmetric positive definite M for every such omega: no spectral estimate is asked of the caller.
 * A one-level hierarchy (MgSetupAggregates with levels = 1) with nuCoarse = 2 is SSOR(omega)-preconditioned CG, MINRES or BiCGStab through
 * SolveMg, SolveMinresMg and SolveBicgstabMg.
 *
 * The COLOURING of a level is deterministic and defined by the data alone.  Row i's neighbours are the columns j != i of its stored
 * entries, whatever their value.
 *   1. the key of a row, 32-bit unsigned arithmetic:
 *        h = i*0x9E3779B1; h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15
 *      rows compare by (h, i).
 *   2. a round: every uncoloured row whose (h, i) is larger than that of each of its uncoloured neighbours takes the smallest colour that
 *      none of its coloured neighbours holds -- "uncoloured" and "coloured" as they stood at the start of the round.
 *   3. rounds repeat until every row is coloured.  The host reads one flag per round.
 *   4. at most 64 colours (one 64-bit mask per row): a row whose neighbours hold all 64 is refused, the message names the level and the row.
 *   5. one device pass then checks every stored entry (i, j), j != i, for colour[i] != colour[j].  It can fail only when the PATTERN is not
 *      structurally symmetric (some j stores i and i does not store j): refused, the message names the level and the row.  The values may be
 *      nonsymmetric.  The check is what makes the in-place sweep free of races, hence deterministic.
 *   The per-colour row lists (rows ascending within a colour) are index bookkeeping and built on the host; no matrix value travels there.
 * A SWEEP visits the colours 0, 1, ... (forward) or in reverse (backward), one launch per colour; within a colour every row i updates in
 * place:  s = the row's sum in stored order from +0.0 of the rounded products a_ik * x[col_k], the diagonal included;  res = b_i - s;
 * t = dinv_i * res;  step = omega * t;  x_i = x_i + step  -- the operations and roundings of the Jacobi sweep, omega the hierarchy's.  The
 * sweeps sum every row in stored order in EVERY mode, whatever its length (several lanes share a row's loads, one order adds the products),
 * and read the level's plain CSR whatever the compression mode; the residual pass and the transfers are those of mode 0 (a residual pass
 * on a level of more than 20 entries a row on average sums by several lanes and a tree unless dot_order = 1, as everywhere in the library).
 * The CYCLE: a level with a map runs nu forward sweeps from x = +0.0, r = b - A x, the indexed restriction, the next level, x += P e, nu
 * backward sweeps; the last level runs nuCoarse sweeps from +0.0, sweep s (0-based) forward when s is even and backward when odd.  The
 * cycle leaves no partial sums of r . z behind: the PCG loop takes them in a pass of its own (16 bytes per row).
 * Returns 0; -1 with MgcgGetLastError() on a refusal, which leaves the hierarchy exactly as it was (usable, its mode unchanged).  Mode 0
 * after mode 1 restores the Jacobi cycle bit for bit; mode 1 twice gives the same colours and the same bits.  Not to be called while a solve
 * on the hierarchy is running. */
int     MgSetSmoother(MgcgMg* mg, int mode);
int     MgSmoother(const MgcgMg* mg);                                     /* the mode in force (0 for NULL) */
int     MgLevelColours(const MgcgMg* mg, int level);                      /* the colours of the level; 0 under mode 0; -1 on a bad level */
/* colourOf[0 .. MgLevelRows(level)-1] = the colour of every row.  Returns 0; -1 with MgcgGetLastError() under mode 0 or on a bad level. */
int     MgLevelCopyColours(const MgcgMg* mg, int level, int colourOf[]);
/* The cycle of an aggregation hierarchy: 0 (default) the V-cycle, 1 Notay's K-cycle with inner = 0 conjugate or inner = 1 minimal-residual
 * steps.  With the unsmoothed piecewise-constant transfer of pairwise aggregates the V-cycle's iteration count grows with the matrix; the
 * K-cycle solves the coarse problem of every level by TWO Krylov steps preconditioned by the cycle, where the V-cycle runs one cycle, and
 * its count stays flat.  The level matrices, maps, smoother and transfers are the V-cycle's; with L + 1 levels the cycle of level l runs 2^l times per
 * application for 1 <= l < L and 2^(L-1) times on the last level.
 *
 * ACCEPTED: aggregation hierarchies (MgSetupAggregation, MgSetupAggregationEx, MgSetupAggregates), one rank, either smoother.
 * REFUSED before a device is asked for (-1, MgcgGetLastError(), the handle unchanged and usable): a null handle; cycle outside {0, 1};
 * inner outside {0, 1}; an ILU(0) handle; a geometric hierarchy (MgSetup / MgSetupParallel); a hierarchy of several ranks.
 *
 * The K STEP runs on level l whenever level l + 1 = C is not the last level (C has a map of its own), where the V-cycle calls
 * cycle(C, b_c) once between the restriction b_c = P^T r and x += P e.  On a hierarchy of one or two levels no level qualifies and the
 * cycle is the V-cycle bit for bit.  Every vector has C's rows.  Every sum is a dot product of the library: in the default mode per-lane
 * and per-workgroup partial sums added in a fixed order (reproducible from run to run), under dot_order = 1 one serial sum left to right
 * from +0.0 of the rounded products.  u(c, v) = c for inner = 0 and v for inner = 1:
 *     c1 = cycle(C, b_c);   v1 = A_C c1   (the level's own product: rows summed as the level's residual pass sums them)
 *     rho1 = sum u1_i * v1_i;   beta1 = sum u1_i * b_c,i                                      (u1 = u(c1, v1))
 *     a1 = beta1 / rho1;   rr_i = b_c,i - p_i with p_i = a1 * v1_i
 *     c2 = cycle(C, rr);   v2 = A_C c2
 *     gamma = sum u2_i * v1_i;   beta = sum u2_i * v2_i;   a2 = sum u2_i * rr_i               (u2 = u(c2, v2))
 *     t = gamma * gamma;   q = t / rho1;   rho2 = beta - q
 *     g = gamma * a2;   d = rho1 * rho2;   h = g / d;   k1 = a1 - h;   k2 = a2 / rho2
 *     e_i = p1_i + p2_i with p1_i = k1 * c1_i and p2_i = k2 * c2_i
 * Every named quantity is one rounded operation on doubles; no product is fused with the sum or difference that takes it.  e takes the
 * place of the V-cycle's coarse result.  (inner = 0 is two steps of CG on A_C e = b_c preconditioned by the cycle, inner = 1 the two-step
 * minimal-residual form: c1^T (b_c - A_C e) = c2^T (b_c - A_C e) = 0, respectively the same with v1 and v2.)
 * BREAKDOWN is decided on the device, with no host read; "finite and > 0" is the library's test 0 < v <= 1.79e308:
 *     rho1 not finite or not > 0:             rr = b_c and e = c1, the V-cycle's answer (b_c = 0 gives e = +0.0, never NaN);
 *     otherwise rho2 not finite or not > 0:   e_i = a1 * c1_i.
 * The second cycle and its product are enqueued in every case: the launch sequence does not depend on the data.  Notay's early exit
 * (no second step when ||rr|| <= 0.25 ||b_c||) would need a data-dependent launch and is not built.
 *
 * WHICH SOLVES: under mode 1 M is no longer one fixed linear map (a1, k1, k2 depend on the vector).  MgApply and SolveGmresMg (flexible by
 * construction) take it.  SolveMg takes it and KEEPS its standard beta = r_new . z_new / r . z: a CPU trial of both on 32^3 .. 64^3 Poisson matrices
 *  saw the same iteration counts with the standard and with the flexible (Polak-Ribiere) beta.  SolveMgParallel, SolveMinresMg, SolveBicgstabMg and MgcgSolveLobpcgMg refuse a handle in mode 1 at
 * entry, before anything is enqueued, with a message that names MgSetCycle; the handle and the caller's vectors stay untouched.
 * STORAGE: every level that is the C of a K step gets four vectors of its rows (the second cycle's spare iterate buffer, so that c1 stays
 * where the first cycle left it, v1, v2 and rr) and 5 x 2048 doubles of partial sums, allocated by mode 1 and freed by mode 0 and MgDestroy.
 * An allocation failure is a refusal that leaves the hierarchy in V mode.
 * Returns 0; -1 on a refusal.  Mode 0 after mode 1 restores the V-cycle bit for bit; mode 1 twice gives the same bits (the second call may
 * change inner).  Not to be called while a solve on the hierarchy is running. */
int     MgSetCycle(MgcgMg* mg, int cycle, int inner);
int     MgCycle(const MgcgMg* mg);                                        /* the mode in force (0 for NULL) */
int     MgCycleInner(const MgcgMg* mg);                                   /* the inner steps in force (0 for NULL and under mode 0) */
/* New VALUES for the pattern an aggregation hierarchy was built from: the numeric half of the set-up alone, for time steppers, Newton and
 * Picard loops and parameter sweeps, which solve a sequence of matrices of one sparsity pattern.  The maps, the pattern of every level,
 * the colours of MgSetSmoother(mg, 1), the vectors of MgSetCycle, the modes, omega, nu, nuCoarse and sigma stay; the values of every
 * level below the first, every D^-1 and dinvUniform / dinvScalar are formed again.
 *
 * THE RESULT is, bit for bit, the hierarchy MgSetupAggregates builds from the new values and the maps of MgLevelCopyAggregates: the same
 * level matrices, the same D^-1, hence the same cycle.  THE MAPS ARE KEPT: it is NOT necessarily the hierarchy the matching of
 * MgSetupAggregation(Ex) would choose for the new values; whether the kept maps still suit them is the caller's judgement (the iteration
 * counts show it).
 *
 * ARGUMENTS: elementsVector holds elementsCount values in the stored order of set-up; elementsCount must equal MgLevelNnz(mg, 0).  It may
 * be the vector the hierarchy was built from, rewritten in place, or another vector: level 0 then points at it from now on and the caller
 * keeps it alive, as at set-up (the solvers still multiply by the vectors THEY are given).  THE CALLER'S PROMISE, not checked: the row
 * offsets and column indices of level 0 are those of set-up, unchanged, in the vectors given then.
 *
 * ACCEPTED: one-rank aggregation hierarchies (MgSetupAggregation, MgSetupAggregationEx, MgSetupAggregates), either strength, either
 * smoother, V or K cycle, one level (only D^-1 changes) or many.  REFUSED before a device is asked for (-1, MgcgGetLastError(), the handle
 * untouched): a null handle or vector; an ILU(0) handle (the message says: MgSetupIlu0 again); a geometric hierarchy (MgSetup again);
 * several ranks; elementsCount != MgLevelNnz(mg, 0); a vector of fewer than elementsCount values.
 *
 * THE SOURCE LISTS.  By the Galerkin contract above every entry q of level l + 1 is sigma times the serial sum, from +0.0, of a fixed
 * list of entries of level l in a fixed order: the entries (i, j) with aggregate(i) = row(q) and aggregate(j) = column(q), members i
 * ascending, each member's entries in stored order.  The first call builds that list for every level that has a map, on the device, from
 * the pattern and the maps alone (no value is read): sources[segmentOffsets[q] .. segmentOffsets[q + 1]) = the stored positions in level l
 * of q's entries in that order -- a stable counting sort of the contract-order entry stream by coarse entry.  The lists
 * (MgLevelNnz(l + 1) + 1 + MgLevelNnz(l) ints per such level) and the shadow buffers below are kept until MgDestroy; MgUpdateBytes tells
 * what they hold.  A handle that never sees this call allocates none of it.
 *
 * THE NUMERIC PASS, one launch per level: C[q] = sigma * (((+0.0 + a[src[o]]) + a[src[o + 1]]) + ...), o from segmentOffsets[q].  One
 * lane sums a segment, serially; no atomic, no reordering, sums that come to zero are kept: the bits do not depend on the grid or on
 * where a tile of the list ends.  Then set-up's diagonal check, D^-1 and its uniformity test on the new values of every level.
 *
 * ALL OR NOTHING.  The new coarse values and the new D^-1 go to shadow buffers (allocated by the first call, then used in turns with the
 * buffers in force) and the pointers change hands only when EVERY level has passed the diagonal check.  A diagonal that is not stored, not
 * finite or not > 0 returns -1 with set-up's words, "level l, row i: the diagonal must be stored, finite and > 0" (the first such level,
 * its smallest such row), and nothing of the handle has changed: with another vector the handle is the old hierarchy, bit for bit; with
 * an in-place rewrite level 0 is whatever the caller wrote, over the OLD coarse levels and the OLD D^-1 -- a usable handle, no longer a
 * Galerkin hierarchy, until a later call succeeds.  After the first call the host reads the levels' flags in one copy and nothing else.
 * Matrix forms of MgcgSetMatrixCompression are those of the new values: every buffer written or given up is reported to the analysis cache
 * and every level is looked up afresh.  Returns 0, -1 on a refusal.  Not to be called while a solve on the hierarchy is running. */
int       MgUpdateValues(MgcgMg* mg, Vector* elementsVector, int elementsCount);
long long MgUpdateBytes(const MgcgMg* mg);                                /* device bytes the source lists and shadow buffers hold; 0 before the first MgUpdateValues, for NULL and for other handles */
/* Level `level`'s list for the product that forms level + 1: segmentOffsets[0 .. MgLevelNnz(level + 1)] and sources[0 .. MgLevelNnz(level) - 1]
 * (host arrays; either may be NULL).  Returns the number of sources; -1 with MgcgGetLastError() before the first MgUpdateValues, on the
 * last level and on a bad level or handle. */
long long MgLevelCopyGalerkinSources(const MgcgMg* mg, int level, int segmentOffsets[], int sources[]);
/* Multicolour ILU(0): M = L U, the incomplete factorisation without fill of A + shift * diag(A) in the COLOUR ORDER, as one more kind of
 * MgcgMg handle.  MgApply, SolveMg, SolveMinresMg, SolveBicgstabMg and SolveGmresMg take it wherever they take a hierarchy: z = M^-1 r is
 * U^-1 L^-1 r.  One rank; any CSR matrix with a stored diagonal in every row, rows in any stored order, no column twice in a row, a
 * structurally symmetric pattern of at most 64 colours; the values may be nonsymmetric.
 *
 * REFUSED before a device is asked for (NULL, MgcgGetLastError()): a null handle; count < 1 or elementsCount < 0; vectors smaller than
 * elementsCount or count + 1; a shift that is not finite or is negative.
 * REFUSED once the arrays have been read, in this order, each naming the smallest such row of A: offsets that do not start at 0, that
 * descend or that end beyond elementsCount; a row that stores a column outside [0, count); an empty row; a row without a stored diagonal;
 * the two refusals of the colouring below; a row that stores a column twice; a pivot that is zero or not finite.  A refusal commits nothing.
 *
 * The COLOURS are those of MgSetSmoother above, by the same code: the same key, the same rounds, at most 64 colours, the same check pass
 * (an unsymmetric pattern is refused); the messages are MgSetSmoother's under this call's name, with "level 0".
 * The ORDER: new row index = the row's position in the list of all rows sorted by (colour, row).  rowOf[new] = old.  The rows of a colour
 * are one contiguous range of new indices and store no entry of each other.
 * The PERMUTED MATRIX B = P (A + shift diag(A)) P^T is stored as CSR with every row sorted by new column.  Its diagonal entry is
 * a_ii + shift * a_ii, the product rounded first (shift = 0: a_ii itself, for every finite a_ii); the other entries are bit copies.
 * The FACTOR is the IKJ ILU(0) of B in place, every product rounded before its subtraction: for new row i ascending, for each stored
 * entry (i, k) with k < i in stored (ascending) order:
 *     l = b_ik * pinv_k, stored as b_ik;   for each stored (k, j) with j > k, ascending: if row i stores column j,  b_ij = b_ij - l * b_kj;
 * and when the row is done pinv_i = 1.0 / b_ii.  "i ascending" is one launch per colour; the bits do not depend on how a colour's rows
 * are spread over lanes.  The pivot flag is read after every colour: the refusal names the smallest row of A, among the rows of the first
 * colour that has one, whose pivot b_ii is zero or not finite, and the pivot's value.
 * The SIGN of the pivots is not judged.  MgIluPivotRange reports the smallest and the largest.  The CG and MINRES forms (SolveMg,
 * SolveMinresMg) need a symmetric positive definite M: A symmetric and ALL pivots positive; shift > 0 -- ILU(0) of A + shift * D -- is the
 * usual remedy where they are not.  SolveBicgstabMg and SolveGmresMg ask nothing of M but that it exists.
 * The APPLICATION z = M^-1 r, r and z in the caller's order, y and t in the new order in the handle's own buffers:
 *     forward, colours ascending:   s = the sum in stored order from +0.0 of the rounded products l_ik * y_k over the row's entries left of
 *                                   its diagonal;   y_i = r[rowOf[i]] - s
 *     backward, colours descending: s = the same sum of u_ij * t_j over the entries right of the diagonal;   t_i = pinv_i * (y_i - s);
 *                                   z[rowOf[i]] = t_i
 * One launch per colour per direction over a contiguous range of rows; the sums are serial in every mode (dot_order changes nothing here).
 * The application leaves no partial sums of r . z behind: the loops take them in a pass of their own, as under MgSetSmoother(mg, 1).
 *
 * The handle has one level: MgLevels = 1, MgLevelRows(0) = count, MgLevelNnz(0) = the entries, MgLevelCopyCsr(0) = A as given.  MgDestroy
 * frees it.  It reads the caller's matrix vectors only during this call.  MgSetSmoother, MgSetInterpolation, MgLevelCopyAggregates,
 * MgLevelCopyColours and MgLevelCopyDinv refuse it with a message that says what the handle is.  A solve checks its row count and its one
 * rank as it checks a hierarchy's. */
MgcgMg* MgSetupIlu0(MgcgBlas* cublas, MgcgSparse* cusparse,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    int elementsCount, int count, double shift);
int     MgIsIlu(const MgcgMg* mg);                                        /* 1 for such a handle, 0 otherwise and for NULL */
int     MgIluColours(const MgcgMg* mg);                                   /* the colours; -1 with a message on another handle */
int     MgIluPivotRange(const MgcgMg* mg, double* smallest, double* largest);   /* 0; -1 with a message on another handle */
/* ms[0 .. 2] = what the set-up took on the host's clock: checks and colouring, building B, factorisation with the pivot range. */
int     MgIluSetupMs(const MgcgMg* mg, double ms[3]);
/* The factor as it stands on the device: values, new columns and count + 1 offsets of B's factor (L strictly left of every row's diagonal,
 * the multipliers; U from the diagonal on, the diagonal entry is the pivot), diagonal[i] = the position of row i's diagonal, rowOf[new] =
 * old.  Any pointer may be NULL (not copied).  Returns the entry count, so a call with all pointers NULL sizes the arrays; -1 with a
 * message on another handle. */
long long MgIluCopyFactor(const MgcgMg* mg, double elements[], int columnIndeces[], int rowOffsets[], int diagonal[], int rowOf[]);
int     MgLevels(const MgcgMg* mg);
/* rows / nnz / grid of level l; copy level l's CSR and D^-1 to host arrays (for tests). */
long long MgLevelRows(const MgcgMg* mg, int level);
long long MgLevelNnz(const MgcgMg* mg, int level);
void    MgLevelCopyCsr(const MgcgMg* mg, int level, double elements[], int columnIndeces[], int rowOffsets[]);
void    MgLevelCopyDinv(const MgcgMg* mg, int level, double dinv[]);
/* z = M^-1 r : one V-cycle from a zero guess (raw device pointers, count = level-0 rows). */
void    MgApply(MgcgMg* mg, const double* r, double* z);
/* Preconditioned CG with the reference's shell and stop rules; zVector is one more work vector. */
int     SolveMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector,
                Vector* ApVector, Vector* pVector, Vector* rVector, Vector* zVector,
                int elementsCount, int count,
                double allowableResidual, int minIteration, int maxIteration, int rule,
                int* iteration, double* residual,
                double* residualTrace, int traceCapacity);

/* ---- one process per GPU: RCCL over xGMI ---- */
/* 128-byte RCCL unique id created on one rank and handed to every rank by the launcher
 * (torch.distributed store / MPI / a file). Returns 0 on success. */
int       MgcgCommGetUniqueId(void* id128);
/* 1 if librccl resolved in this process with every entry point the library binds, else 0 (MgcgGetLastError says why).
 * ncclCommInitRank is collective: launchers agree on this (and on one device per local rank) over their own channel
 * BEFORE any rank calls MgcgCommInitRank, so that a rank that cannot enter it never leaves the others blocked inside. */
int       MgcgRcclAvailable(void);
MgcgComm* MgcgCommInitRank(const void* id128, int nranks, int rank);
void      MgcgCommDestroy(MgcgComm* comm);
/* ONE process driving ndev devices, one host thread per device -- the shape of the reference's ConjugateGradientParallelGpu
 * (Mgcg/cuBlas/Mgcg/ConjugateGradientParallelGpu.cs:264-324: every device of the process; :424-565: a Parallel.For per phase).
 * Forms the ndev communicators of devices 0 .. ndev-1 at once, from the calling thread (ncclGroupStart / ndev x
 * ncclCommInitRank / ncclGroupEnd): comms[d] is rank d of ndev and belongs to device d.  Call it before the devices'
 * handles and vectors are created.  Afterwards thread d calls SetDevice(d) and SolveParallel / MgSetupParallel /
 * SolveMgParallel(comms[d], ...); all ndev calls must be in flight together (they meet in collectives).
 * With fewer physical devices than ndev (MGCG_VIRTUAL_DEVICES, tests) the communicators share an in-process loopback group;
 * ndev == 1 gives a single-rank communicator.  Returns 0, or -1 with MgcgGetLastError() and every comms[d] NULL. */
int       MgcgCommInitAll(MgcgComm* comms[], int ndev);
/* "rccl", "loopback", "callbacks", "single" (one rank, no transport) or "none" (NULL). */
const char* MgcgCommTransport(const MgcgComm* comm);
/* Device-side cost of one collective step of the multi-rank loop on this communicator's stream: `reps` back-to-back
 *   what = 0  all-reduces (sum) of `count` doubles (count <= 8),
 *   what = 1  halo exchanges: one grouped send/recv of `count` doubles with every other rank (with itself on one rank),
 *   what = 2  fork / join pairs of the overlap schedule (event record + stream wait on the side stream and back),
 *   what = 3  empty single-workgroup kernel launches (the price of a kernel boundary on this stream),
 *   what = 4  the stencil's halo exchange: one grouped send/recv of `count` doubles with ranks rank - 1 and rank + 1 only,
 * timed with HIP events around the batch; returns microseconds per repetition (NaN on error -- and, without an error message, for
 * what = 1 / 4 on a transport without RCCL: host-staged planes travel through the launcher, there is nothing to time on the device).
 * Collective: every rank of the communicator must make the same call. */
double    MgcgCommProbe(MgcgComm* comm, int what, int count, int reps);
int       MgcgCommRank(const MgcgComm* comm);
int       MgcgCommSize(const MgcgComm* comm);
/* In-process loopback transport: N ranks of ONE process (host threads, e.g. MGCG_VIRTUAL_DEVICES on one GPU)
 * exchange through host memory behind a barrier.  For testing the multi-rank logic where RCCL cannot form a
 * communicator (it needs one device per rank); every rank must make the same sequence of solver calls. */
typedef struct MgcgLoopback MgcgLoopback;
MgcgLoopback* MgcgLoopbackCreate(int nranks);
void          MgcgLoopbackDestroy(MgcgLoopback* group);
MgcgComm*     MgcgCommInitLoopback(MgcgLoopback* group, int rank);
/* Host-staged transport through callbacks of the launcher (e.g. torch.distributed / MPI on host memory): a fallback for
 * hosts where RCCL cannot form a communicator, and a way to drive the multi-rank loop from any message layer.
 *   allGather(mine, all, user):   all[4*q .. 4*q+3] = the four int64 of rank q  (every rank's `mine`, rank order)
 *   allReduce(values, count, user): values[i] = sum over ranks, in place, the SAME bits on every rank
 *   exchange(nranks, sendBufs, sendCounts, recvBufs, recvCounts, user): for every peer q with sendCounts[q] > 0 send
 *       sendBufs[q][0 .. sendCounts[q]) to q, with recvCounts[q] > 0 receive into recvBufs[q]; returns when all arrived.
 * All buffers are host memory owned by the library; the callbacks are invoked from the thread that calls the solver. */
typedef void (*MgcgAllGatherFn)(const long long mine[4], long long all[], void* user);
typedef void (*MgcgAllReduceFn)(double values[], int count, void* user);
typedef void (*MgcgExchangeFn)(int nranks, const double* const sendBufs[], const long long sendCounts[],
                               double* const recvBufs[], const long long recvCounts[], void* user);
MgcgComm*     MgcgCommInitCallbacks(int nranks, int rank, MgcgAllGatherFn allGather, MgcgAllReduceFn allReduce, MgcgExchangeFn exchange, void* user);
/* sum of one double over all ranks (test / bootstrap helper; blocking). */
double    MgcgCommAllReduceSum(MgcgComm* comm, double value);
/* The whole multi-rank CG of ConjugateGradientParallelGpu.Solve (ConjugateGradientParallelGpu.cs:424-565)
 * run natively: this rank owns rows [offsetForDevice, +countForDevice) set up by Initialize; pVector is
 * full length (count).  Halo = the entries of p in [minJ, offset) and [offset+count, maxJ] (exchanged with
 * grouped ncclSend/ncclRecv between the ranks that own them), dot products = local partial + ncclAllReduce.
 * comm == NULL means a single rank.  Same outputs and rules as SolveEx. */
int SolveParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector,
                  Vector* ApVector, Vector* pVector, Vector* rVector,
                  int count, int countForDevice, int offsetForDevice, int elementsCountForDevice,
                  int minJ, int maxJ,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual,
                  double* residualTrace, int traceCapacity);

/* Multi-rank preconditioned CG: SolveParallel with the V-cycle of an MgSetupParallel hierarchy (zVector: local work vector). */
int SolveMgParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* zVector,
                    int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                    double allowableResidual, int minIteration, int maxIteration, int rule,
                    int* iteration, double* residual, double* residualTrace, int traceCapacity);

/* ---- Jacobi-preconditioned CG for general CSR matrices (any SPD matrix with a positive diagonal; one rank or several) ---- */
/* dinv[i] = 1 / a_ii for the local rows [offsetForDevice, +countForDevice): a_ii is the first stored entry of local row i whose column is
 * offsetForDevice + i, wherever it sits in the row (rows need not be sorted).  A row without a stored diagonal -- an empty row included --
 * or with a diagonal that is not finite and > 0 makes the call fail: it returns -1, MgcgGetLastError names the first such row, and
 * dinvVector must not be handed to a solve.  The check runs on the device and is read back once; the call is ordered with the handle's
 * other work.  Returns 0 on success. */
int MgcgJacobiSetup(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    int elementsCount, int countForDevice, int offsetForDevice, Vector* dinvVector);
/* SolveEx with the preconditioner M = diag(A): z = dinv * r, alpha = r.z / p.Ap, beta = r.z_new / r.z, p = z + beta p.  The five stop
 * rules, the trace, *iteration, *residual and the status codes are SolveEx's and test the TRUE residual: sqrt(r.r), max|r| under
 * MGCG_RULE_HANDMADECL, r.r against the true r0.r0 under MGCG_RULE_VIENNACL.  dinvVector: what MgcgJacobiSetup wrote (count entries).
 * No z vector exists: both vector passes of an iteration form z_i = dinv_i * r_i themselves (one rounded product, never fused with the
 * add that follows), so an iteration is the product plus two launches, as SolveEx's, at 80 bytes per row of vector traffic against 64.
 * Rounding contract: r = r + (-alpha) Ap with the product rounded first; the terms of r.r and r.z are r_i * r_i and r_i * z_i of the
 * rounded r; p = z + beta p with both products rounded first.  Under dot_order = 1 every dot of the loop is a serial left-to-right sum.
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update (x_defer) and the
 * placement draw do not apply. */
int SolveJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                int elementsCount, int count,
                double allowableResidual, int minIteration, int maxIteration, int rule,
                int* iteration, double* residual, double* residualTrace, int traceCapacity);
/* SolveParallel with the same preconditioner; dinvVector holds the local rows (the diagonal needs no halo).  r.r and r.z travel in one
 * all-reduce of two doubles.  A rank whose MgcgJacobiSetup failed passes dinvVector = NULL: every rank then returns MGCG_ERROR and
 * nobody waits in a collective.  MGCG_RULE_HANDMADECL is single-rank only, as in SolveParallel. */
int SolveJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector,
                        int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* residualTrace, int traceCapacity);

/* ---- Single-reduction CG (Chronopoulos-Gear): the same Krylov method with ONE global sum per iteration (one rank or several) ---- */
/* SolveEx / SolveJacobi with the product moved in front of both sums.  One rank: an iteration is the product and ONE fused vector pass
 * (two launches where SolveEx has three).  Several ranks: the product, one small launch, one all-reduce of 3 doubles (2 without
 * dinvVector) and the pass -- three launches and one all-reduce where SolveParallel has five and two.  The price is one more vector
 * (s = A p, kept by recurrence) and 72 bytes per row of pass traffic against 64 (88 against 80 with dinvVector): a loop for
 * latency-bound systems and for ranks, not for systems whose iteration is memory traffic.  Other bits than SolveEx's, the same method.
 * Method (dinv = 1 / diag(A), or all ones when dinvVector is NULL):
 *   start   r = b - A x ;  u = dinv r ;  rr0 = rr = r.r ;  gamma = r.u ;  w = A u ;  delta = w.u
 *   body k  k = 0:  beta = 0 ;  alpha = gamma / delta
 *           k > 0:  beta = gamma / gamma_old ;  t = beta*gamma ;  q = t / alpha_old ;  den = delta - q ;  alpha = gamma / den
 *           p = u + beta p ;  s = w + beta s          (k = 0: p = u, s = w; the old p and s are not read)
 *           x = x + alpha p ;  r = r + (-alpha) s ;  u = dinv r
 *           gamma_old = gamma ; alpha_old = alpha ;  gamma = r.u ;  rr = r.r
 *           w = A u ;  delta = w.u
 * Rounding contract: every product goes into a double of its own before the add that follows it, nothing is fused; the scalars are
 * evaluated in exactly the order written; per element bp = beta*p_i ; p_i = u_i + bp ; bs = beta*s_i ; s_i = w_i + bs ; ap = alpha*p_i ;
 * x_i = x_i + ap ; as = (-alpha)*s_i ; r_i = r_i + as ; u_i = dinv_i*r_i; the terms of the sums are r_i*r_i and r_i*u_i of the rounded r
 * and u, and w_i*u_i; without dinvVector u is r.  Under dot_order = 1 delta, gamma and rr are serial left-to-right sums and ranks add in
 * rank order: the whole loop is then a fixed sequence of IEEE operations.
 * Stop: the four 2-norm rules of SolveEx on the true (rr, rr0); MGCG_RULE_HANDMADECL is refused with MGCG_ERROR before anything is enqueued.
 * The decision on body k's rr is taken at the one reduction point, behind the next product: one product at the very end is wasted, and x is
 * the iterate whose residual was judged.  *iteration, *residual, the trace (entry k: body k's residual; sqrt(rr / rr0) under
 * MGCG_RULE_VIENNACL) and the status mean what they mean for SolveEx.  MGCG_RULE_SIMPLE starts from x = 0.
 * Breakdown: delta (k = 0) or den not finite or <= 0, or an alpha that is not finite, ends the loop with MGCG_NONFINITE before body k's
 * updates: x keeps the last completed iterate, *iteration = k, and *residual and trace entry k repeat that iterate's residual.
 *   ApVector, pVector, rVector, sVector   work space (count entries each; the layout is internal: w, u, r, s).  The direction p lives
 *                   on the handle's workspace (one more vector of count entries, allocated at the first call and kept).  On return
 *                   rVector holds the recurrence residual.
 *   dinvVector      what MgcgJacobiSetup wrote, or NULL for the unpreconditioned loop
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update (x_defer) and the
 * placement draw do not apply.  Out of scope: the V-cycle as preconditioner, the block, shifted and mixed variants, and hiding the
 * all-reduce behind the product (pipelined CG). */
int SolveSingleReduce(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* sVector, Vector* dinvVector /* may be NULL */,
                      int elementsCount, int count,
                      double allowableResidual, int minIteration, int maxIteration, int rule,
                      int* iteration, double* residual, double* residualTrace, int traceCapacity);
/* The same on a row partition, shaped after SolveJacobiParallel: pVector is full length (count entries; it holds u, whose halo is exchanged
 * before every product, in line -- the overlap schedule is not used by this loop), the other vectors hold the local rows.  A rank without
 * rows takes part in every collective.  Every rank passes a dinvVector or none does: that is not checked (the ranks would disagree on the
 * length of the all-reduce); every other unusable argument on one rank makes every rank return MGCG_ERROR, as in SolveParallel. */
int SolveSingleReduceParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                              Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* sVector, Vector* dinvVector /* may be NULL */,
                              int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                              double allowableResidual, int minIteration, int maxIteration, int rule,
                              int* iteration, double* residual, double* residualTrace, int traceCapacity);

/* ---- MINRES: symmetric indefinite and shifted systems (A - shift I) x = b (one rank or several) ---- */
/* Paige and Saunders' minimum-residual method.  A is symmetric CSR of any inertia, shift is finite and of any sign (0: plain MINRES).
 * Every other solver here needs a positive definite matrix and returns MGCG_NONFINITE when p.Ap <= 0; this one does not.  It runs the
 * Lanczos recurrence of CG at the plain loop's cost structure -- one product and two global sums per iteration -- and minimises || r ||_2,
 * the very norm every stop rule of this library judges, over the Krylov space: on a definite matrix it never needs more iterations than CG
 * to the same rule, and its residual trace never increases.  The Lanczos vectors of A - shift I are those of A, so the shift never
 * touches a vector inside the loop: it enters the scalar alpha only.  One rank: three launches per iteration (the product and two fused
 * vector passes, 32 and 64 bytes per row).
 * Method:
 *   start   (MGCG_RULE_SIMPLE: x := 0)
 *           t = b - A x  (row i of A x summed as the product sums it, then b_i - acc) ;  r_i = t_i + shift*x_i ;  rr0 = r.r ;  beta1 = sqrt(rr0)
 *           rr0 not finite or == 0  ->  MGCG_NONFINITE at iteration 0, x untouched
 *           v = r*(1/beta1) ;  beta = 0 ;  cs = -1 ;  sn = 0 ;  dbar = 0 ;  eps = 0 ;  phibar = beta1 ;  trace[0] = beta1 (sqrt(rr0/rr0) under
 *           MGCG_RULE_VIENNACL)
 *   body k  q = A v ;  delta = v.q
 *   pass A  y_i = (q_i - delta*v_i) - beta*vprev_i      (k = 0: the beta term is not formed, vprev is not read) ;  yy = y.y
 *   pass B  alpha = delta - shift ;  betan = sqrt(yy)
 *           oldeps = eps ;  dl = cs*dbar + sn*alpha ;  gbar = sn*dbar - cs*alpha ;  eps = sn*betan ;  dbar = -(cs*betan)
 *           gamma = sqrt(gbar*gbar + betan*betan) ;  ig = 1/gamma ;  cs = gbar*ig ;  sn = betan*ig ;  phi = cs*phibar ;  phibar = sn*phibar
 *           gamma, ig or phi not finite, or gamma == 0  ->  MGCG_NONFINITE reported for iteration k + 1, x and the directions unchanged by this body
 *           w_i = ((v_i - oldeps*w1_i) - dl*w2_i)*ig    (k = 0: w1, w2 not read; k = 1: w1 not read) ;  x_i = x_i + phi*w_i
 *           vnext_i = y_i*(1/betan)                     (not formed when betan == 0)
 *           rr = phibar*phibar is judged by the rule's stop test against rr0 as the residual of iteration k + 1
 *           betan == 0: the Krylov space is exhausted; the loop ends after this body with the rule's status if it stops, else MGCG_OK
 *           (vprev, v) := (v, vnext) ;  (w1, w2) := (w2, w) ;  beta := betan
 *   end     one more product: t = b - A x ;  r_i = t_i + shift*x_i into rVector ;  *trueResidual = sqrt(r.r)
 * Rounding contract: every product goes into a double of its own before the add or subtraction that follows it, nothing is fused; the
 * scalars are evaluated in exactly the order written (1/beta1, 1/betan and ig are formed once and multiplied); the terms of the sums are
 * v_i*q_i, y_i*y_i and r_i*r_i of the rounded y and r.  Under dot_order = 1 every sum is serial left to right and ranks add in rank order:
 * the whole loop is then a fixed sequence of IEEE operations (tests/test_minres_host.py restates it in numpy).
 * Stop: the four 2-norm rules of SolveEx on (rr, rr0) with rr the recurrence's phibar^2; MGCG_RULE_HANDMADECL is refused (the recurrence
 * carries no max|r|).  *iteration, *residual and the trace (entry 0: the first residual; entry k + 1: |phibar| after body k; sqrt(rr / rr0)
 * under MGCG_RULE_VIENNACL) show the recurrence's figure.  phibar can drift from the true residual -- forced past convergence on a 300-row tridiagonal system
 * it underflows to 0 after n iterations where b - A x is 6e-15 -- and a caller of an indefinite solver needs the true figure: the closing
 * product runs whenever the loop ended without MGCG_ERROR, breakdown included, and *trueResidual (may be NULL) is || b - (A - shift I) x ||_2.
 * A breakdown (shift an eigenvalue met by the Krylov space, or values that are not finite) repeats the last judged residual in *residual
 * and its trace entry.
 *   ApVector        work space (count entries): q
 *   pVector, rVector  the two Lanczos buffers, rotated by pointer per body (count entries each).  On return the first count entries of
 *                   rVector hold the true residual, whatever the parity of the rotation
 *   w1Vector, w2Vector   work space (count entries each): the two direction buffers, rotated the same way
 * Refused with MGCG_ERROR, a message and nothing enqueued: a shift that is not finite, MGCG_RULE_HANDMADECL, an unknown rule, a null
 * handle, a vector that is too small.
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update (x_defer), the placement
 * draw and the overlap schedule do not apply.  Preconditioning: SolveMinresJacobi and SolveMinresMg below.  Out of scope: the block and mixed
 * combinations, the C++ twin under host/, and MINRES-QLP for singular systems. */
int SolveMinres(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* w1Vector, Vector* w2Vector,
                int elementsCount, int count, double shift,
                double allowableResidual, int minIteration, int maxIteration, int rule,
                int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
/* The same on a row partition, shaped after SolveSingleReduceParallel.  BOTH Lanczos buffers, pVector and rVector, are full length (count
 * entries): rows gather v, whose halo is exchanged in line before every product (the overlap schedule is not used by this loop); the other
 * vectors hold the local rows.  delta and yy each travel in one all-reduce of one double (two per iteration, as in SolveParallel), the
 * closing r.r in one more.  On return the first countForDevice entries of rVector hold this rank's rows of the true residual, and
 * *trueResidual is the global figure on every rank.  A rank without rows takes part in every collective.  Every rank passes the same
 * shift: that is not checked; every other unusable argument on one rank makes every rank return MGCG_ERROR, as in SolveParallel. */
int SolveMinresParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* w1Vector, Vector* w2Vector,
                        int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ, double shift,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- preconditioned MINRES: (A - shift I) x = b with the diagonal or the V-cycle as preconditioner ---- */
/* Paige and Saunders' MINRES with a symmetric POSITIVE DEFINITE preconditioner M, for the systems SolveMinres takes: A symmetric CSR of any
 * inertia, shift finite and of any sign.  M is the diagonal of MgcgJacobiSetup (SolveMinresJacobi*: z = dinv*r is formed per element inside
 * the passes, there is no z vector) or the V-cycle of any one-rank hierarchy -- MgSetup, MgSetupAggregation, MgSetupAggregates -- whose
 * level 0 has `count` rows (SolveMinresMg: what SolveMg enqueues, r -> zVector).  The hierarchy need not be built from the solved matrix: a
 * caller may build it for A + |shift| I, which is positive definite where A - shift I is not; only the row count is checked.  One
 * application of M^-1 per iteration, still two global sums.  Below z means M^-1 applied.
 * Method:
 *   start   (MGCG_RULE_SIMPLE: x := 0)
 *           t = b - A x  (as in SolveMinres) ;  r2_i = t_i + shift*x_i ;  z = M^-1 r2 ;  bz = r2.z
 *           bz not finite or <= 0  ->  MGCG_NONFINITE at iteration 0, x untouched (a negative bz: the message says that the preconditioner is
 *           not positive definite)
 *           beta = beta1 = sqrt(bz) ;  v = z*(1/beta1) ;  vv = v.v ;  oldb = 0 ;  cs = -1 ;  sn = 0 ;  dbar = 0 ;  eps = 0 ;  phibar = beta1 ;
 *           trace[0] = beta1 (sqrt(bz/bz) under MGCG_RULE_VIENNACL)
 *   body k  q = A v ;  vq = v.q                                   (the plain loop's product)
 *   pass A  alpha = vq - shift*vv ;  c1 = beta/oldb (k > 0) ;  c2 = alpha/beta            (the two quotients are formed once per body)
 *           y_i = q_i - shift*v_i                                 (shift == 0: the term is not formed, v is not read)
 *           y_i = y_i - c1*r1_i                                   (k = 0: not formed, r1 is not read)
 *           rn_i = y_i - c2*r2_i ,  written over r1
 *           Jacobi: z_i = dinv_i*rn_i is formed per element ;  rz = sum rn_i*z_i
 *           V-cycle: the hierarchy's cycle rn -> zVector, then one dot launch for rz = rn.z
 *   pass B  rz < 0 or not finite  ->  MGCG_NONFINITE reported for iteration k + 1, x and the directions unchanged by this body
 *           betan = sqrt(rz) ;  SolveMinres's rotation with this alpha and betan, operation for operation, with its breakdown test
 *           w_i = ((v_i - oldeps*w1_i) - dl*w2_i)*ig over w1 ;  x_i = x_i + phi*w_i
 *           v_i := z_i*(1/betan) IN PLACE                         (Jacobi: z_i formed again from rn_i and dinv_i ;  not formed when betan == 0)
 *           vv = sum v_i*v_i of the new v
 *           rr = phibar*phibar is judged against bz as the residual of iteration k + 1 ;  betan == 0 ends the loop as in SolveMinres
 *           (r1, r2) := (r2, rn) ;  (w1, w2) := (w2, w) ;  oldb := beta ;  beta := betan
 *   end     SolveMinres's closing product: b - (A - shift I) x into rVector, its 2-norm in *trueResidual
 * Rounding contract: SolveMinres's -- every product (shift*vv, shift*v_i, c1*r1_i, c2*r2_i, dinv_i*rn_i, rn_i*z_i, z_i*(1/betan), v_i*v_i, ...)
 * goes into a double of its own before the add or subtraction that follows it, nothing is fused, the scalars are evaluated in the order
 * written.  Under dot_order = 1 every sum is serial left to right and ranks add in rank order (tests/test_pminres_host.py restates the loop
 * in numpy); the V-cycle is MgApply's fixed sequence of operations in either mode.
 * WHAT THE STOP RULE JUDGES: phibar is || r || in the M^-1 NORM, sqrt(r . M^-1 r) -- the quantity preconditioned MINRES minimises -- not the
 * 2-norm.  The four 2-norm rules of SolveEx are applied to (phibar^2, beta1^2 = bz); *iteration, *residual and the trace show that figure
 * (it never increases); MGCG_RULE_HANDMADECL is refused.  *trueResidual (may be NULL) remains the plain 2-norm || b - (A - shift I) x ||_2
 * from the closing product, which runs whenever the loop ended without MGCG_ERROR.  The two norms differ by the conditioning of M: a
 * caller who needs the 2-norm below a level looks at *trueResidual (on this project's test systems the relative true residual was up to
 * 2.2 x the relative phibar at the stop).  A 2-norm recurrence of the true residual would cost one more vector; it is not carried.
 *   ApVector        work space (count entries): q
 *   pVector         v, the one full-length buffer (count entries), overwritten in place by pass B
 *   rVector, r1Vector   the two residual buffers, rotated by pointer per body (local rows).  On return rVector holds the true residual,
 *                   whatever the parity of the rotation
 *   w1Vector, w2Vector   the two direction buffers, rotated the same way (local rows)
 *   dinvVector      what MgcgJacobiSetup wrote (local rows) ;  zVector: work space of the V-cycle form (count entries)
 * One rank, Jacobi: three launches per iteration; the two passes move 48 (40 with shift == 0) and 72 bytes per row.  V-cycle: the cycle
 * and one dot launch more.
 * Refused with MGCG_ERROR, a message and nothing enqueued: everything SolveMinres refuses; a null dinvVector, mg or zVector; an r1, z or
 * dinv vector that is too small; a hierarchy whose level 0 does not have `count` rows; a hierarchy of several ranks.
 * Out of scope: the V-cycle on several ranks, Chebyshev as M, a true 2-norm stop, the block and mixed variants, the C++ twin under host/. */
int SolveMinresJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                      Vector* dinvVector,
                      int elementsCount, int count, double shift,
                      double allowableResidual, int minIteration, int maxIteration, int rule,
                      int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
/* The same on a row partition, shaped after SolveMinresParallel.  Only pVector (v) is full length and has its halo exchanged, in line before
 * every product; every other vector holds the local rows.  {vq, vv} travel in ONE all-reduce of two doubles and rz in one more (two per
 * iteration, as in SolveParallel), the first bz and the closing r.r in one each.  A rank without rows takes part in every collective.  A
 * rank whose dinvVector is NULL (its MgcgJacobiSetup failed) makes every rank return MGCG_ERROR, as in SolveJacobiParallel; every rank
 * passes the same shift: that is not checked. */
int SolveMinresJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                              Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                              Vector* dinvVector,
                              int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ, double shift,
                              double allowableResidual, int minIteration, int maxIteration, int rule,
                              int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
/* The V-cycle form (one rank). */
int SolveMinresMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* r1Vector, Vector* w1Vector, Vector* w2Vector,
                  Vector* zVector,
                  int elementsCount, int count, double shift,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- BiCGStab: nonsymmetric systems A x = b, plain and Jacobi-preconditioned (one rank or several) ---- */
/* Van der Vorst's BiCGStab.  A is ANY CSR matrix: every other solver here takes a symmetric one, and on A != A^T the CG loops break down or
 * return a wrong x and MINRES is not defined.  The method needs only A v (no transpose product, no new matrix form) and fixed storage.  It is
 * right-preconditioned with M = I (SolveBicgstab*) or M = diag(A) (SolveBicgstabJacobi*, dinvVector from MgcgJacobiSetup, which refuses a row
 * without a positive finite stored diagonal): r stays the residual of the system itself, and every stop rule judges its 2-norm, as
 * everywhere else in the library.  A body costs two products and three global sums; one rank: six launches per body (two products, four
 * vector passes of 24 + 8 + 56 + 32 = 120 bytes per row without the diagonal, 40 + 8 + 64 + 48 = 160 with it).
 * Method: d_i is dinv_i when a diagonal is given and 1 otherwise; with d = 1 the multiplication is not performed and no hatted copy is stored.
 *   start   (MGCG_RULE_SIMPLE: x := 0)
 *           r = b - A x  (row i of A x summed as the product sums it, then b_i - acc) ;  rhat = r ;  p = r ;  phat_i = d_i*p_i ;  rho = rr0 = r.r
 *           rr0 == 0 or not finite  ->  MGCG_NONFINITE at iteration 0, x untouched (as SolveMinres)
 *   body k  v = A phat ;  sigma = rhat.v
 *           sigma == 0 or not finite, or alpha = rho/sigma not finite  ->  MGCG_NONFINITE for iteration k + 1, x unchanged by this body
 *           s_i = r_i - alpha*v_i ;  shat_i = d_i*s_i
 *           t = A shat ;  theta = t.s ;  tau = t.t
 *           omega = (tau == 0) ? 0 : theta/tau ;  omega not finite  ->  MGCG_NONFINITE for iteration k + 1, x unchanged by this body
 *           x_i = (x_i + alpha*phat_i) + omega*shat_i ;  r_i = s_i - omega*t_i ;  rr = r.r ;  rhon = rhat.r
 *           rr is judged by the rule's stop test against rr0 as the residual of iteration k + 1
 *           not stopped and (omega == 0 or rhon == 0 or rhon not finite)  ->  MGCG_NONFINITE for iteration k + 1 (x IS this body's iterate)
 *           beta = (rhon/rho)*(alpha/omega) ;  p_i = r_i + beta*(p_i - omega*v_i) ;  phat_i = d_i*p_i ;  rho = rhon
 *   end     one more product: rVector = b - A x ;  *trueResidual = sqrt(r.r)      (whenever the loop ended without MGCG_ERROR)
 * Rounding contract, the same as the other loops: every product (alpha*v_i, d_i*s_i, alpha*phat_i, omega*shat_i, omega*t_i, omega*v_i,
 * beta*(p_i - omega*v_i), d_i*p_i, and the terms rhat_i*v_i, s_i*t_i, t_i*t_i, r_i*r_i, rhat_i*r_i of the rounded vectors) goes into a double
 * of its own before the add or subtraction that follows it, nothing is fused; the scalars are evaluated in exactly the order written (the
 * two quotients of beta are formed, then multiplied).  Under dot_order = 1 every sum is serial left to right and ranks add in rank order:
 * the whole loop is then a fixed sequence of IEEE operations (tests/test_bicgstab_host.py restates it in numpy).
 * Stop: the four 2-norm rules of SolveEx on (rr, rr0); MGCG_RULE_HANDMADECL is refused (the loop carries no max|r|).  *iteration, *residual
 * and the trace (entry 0: the first residual; entry k + 1: sqrt(rr) after body k, sqrt(rr / rr0) under MGCG_RULE_VIENNACL) show the
 * recurrence's figure; a breakdown repeats the last judged figure in *residual and its trace entry.  The recurrence's r can drift from
 * b - A x (classical BiCGStab drift: on the tridiagonal matrix (-1.9, 2, -0.1) the recurrence reaches the level while the true residual has
 * grown by tens of orders of magnitude), so the closing product runs whenever the loop ended without MGCG_ERROR, breakdown included, and
 * *trueResidual (may be NULL) is || b - A x ||_2: a caller of a nonsymmetric solver looks there.
 *   ApVector        with a diagonal: p, the unhatted direction (count entries) ;  without: not used by the loop
 *   pVector         phat, the first buffer the products gather from (count entries) ;  without a diagonal p itself
 *   rVector         r ;  with a diagonal s is written over it between pass S and pass X (the two are never alive together).  On return its
 *                   first count entries hold the true residual b - A x
 *   vVector, tVector   v = A phat and t = A shat (count entries each)
 *   sVector         shat, the second buffer the products gather from (count entries) ;  without a diagonal s itself
 *   rhatVector      the shadow residual, fixed after the start (count entries)
 * Refused with MGCG_ERROR, a message and nothing enqueued: MGCG_RULE_HANDMADECL, an unknown rule, a null handle, a vector that is too small.
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update (x_defer), the placement
 * draw and the overlap schedule do not apply.  The V-cycle as preconditioner: SolveBicgstabMg below; BiCGStab(l): SolveBicgstabL below; GMRES(m): SolveGmres below.  Out of scope:
 * residual replacement, the block and mixed combinations, the C++ twin under host/. */
int SolveBicgstab(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                  Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                  Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                  Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                  int elementsCount, int count,
                  double allowableResidual, int minIteration, int maxIteration, int rule,
                  int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
int SolveBicgstabJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                        Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                        Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector, Vector* dinvVector,
                        int elementsCount, int count,
                        double allowableResidual, int minIteration, int maxIteration, int rule,
                        int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
/* The same on a row partition, shaped after SolveMinresParallel.  pVector and sVector are full length (count entries): rows gather phat and
 * shat, and each has its halo exchanged in line before its product (the overlap schedule is not used by this loop); every other vector
 * holds the local rows (countForDevice entries).  A body has three reduction points: sigma, then {theta, tau}, then {rr, rhon} -- three
 * all-reduces of 1, 2 and 2 adjacent doubles -- and the first and the closing r.r take one each.  On return the first countForDevice entries
 * of rVector hold this rank's rows of the true residual, and *trueResidual is the global figure on every rank.  A rank without rows takes
 * part in every collective.  An unusable argument on one rank (in the Jacobi form also a NULL dinvVector: its MgcgJacobiSetup failed) makes
 * every rank return MGCG_ERROR, as in SolveParallel. */
int SolveBicgstabParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                          Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                          Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                          Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                          int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                          double allowableResidual, int minIteration, int maxIteration, int rule,
                          int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
int SolveBicgstabJacobiParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                                Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                                Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                                Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector, Vector* dinvVector,
                                int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                                double allowableResidual, int minIteration, int maxIteration, int rule,
                                int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* The V-cycle form (one rank): SolveBicgstab's method, line for line, right-preconditioned with the V-cycle of any one-rank hierarchy --
 * MgSetup, MgSetupAggregation, MgSetupAggregates -- whose level 0 has `count` rows: phat = M^-1 p and shat = M^-1 s are what MgApply enqueues
 * (p -> pVector, s -> sVector) instead of a product per element.  Right-preconditioned BiCGStab asks nothing of M but that it is one fixed
 * linear map: M need be neither symmetric nor positive definite, so the hierarchy may be built from the nonsymmetric matrix itself (the
 * set-up sums whole rows and the cycle multiplies by the level matrices as stored: the box maps of MgSetup and of MgSetupAggregates build
 * the level matrices of the numpy yardstick from A != A^T, bit for bit, and so does MgSetupAggregation; its matching pairs rows on MUTUAL
 * picks, so where every row's heaviest coupling points the same way -- an upwinded stencil, central differences at a cell Peclet number
 * near 1 -- nobody is picked back, no level is built and the cycle is nuCoarse Jacobi sweeps on the matrix: still a fixed linear map, and
 * the caller's own aggregates are the way to a real hierarchy there), or from any other matrix with `count` rows, (A + A^T)/2 for instance.
 * Only the row count is checked.
 * Start, breakdown rules, stop rules, trace, the closing product and *trueResidual are SolveBicgstab's, and so is the rounding contract;
 * under dot_order = 1 every sum is serial, and the cycle is MgApply's fixed sequence of operations in either mode
 * (tests/test_bicgstab_mg_host.py restates the loop in numpy).
 * A body is, in this order: the cycle p -> phat ;  v = A phat with sigma = rhat.v ;  pass S (alpha, s over r; no shat written) ;  the cycle
 * s -> shat ;  t = A shat with theta = s.t, the sum taken with the UNHATTED s ;  tau = t.t ;  pass X (the general form: reads x, phat, shat,
 * s, t, rhat) ;  pass P (the stop decision, beta, p; no phat written).  The first cycle of body 0 follows the start, which leaves phat alone.
 * The passes move 24 + 8 + 64 + 32 = 128 bytes per row, beside 120 and 160.
 * The vectors are the Jacobi form's seven, in the same roles; there is no z vector:
 *   ApVector        p, the unhatted direction (count entries), the input of the first cycle
 *   pVector         phat, the first cycle's output and the buffer the first product gathers from
 *   rVector         r ;  s is written over it between pass S and pass X, and is the input of the second cycle.  On return: b - A x
 *   sVector         shat, the second cycle's output and the buffer the second product gathers from
 *   vVector, tVector, rhatVector   as in SolveBicgstabJacobi
 * WHY A BODY ENQUEUED BEHIND THE STOP CHANGES NOTHING.  The host enqueues bodies ahead of the device's stop.  Both cycles and both products
 * take the live stop flag as their gate; pass S copies the flag, as it found it, for pass X and pass P.  (1) Pass P raised the flag: every
 * kernel of the next body's first cycle returns at the gate, the product is skipped, pass S records the flag and returns, the second cycle,
 * the second product and the tau pass return at the gate, pass X and pass P return at the recorded flag -- no vector, no scalar and no trace
 * entry is written.  (2) Pass S met a breakdown of sigma (flag still down): it wrote no vector, so rVector still holds r; the second cycle runs
 * on that r and writes sVector and the hierarchy's own iterates only, the product and the tau pass write tVector and partial sums only, pass X
 * returns at pass S's note, and pass P publishes the breakdown and raises the flag.  x and r are this body's predecessors', as in
 * SolveBicgstab; sVector and tVector are read by nothing afterwards (the closing product goes through pVector into rVector).  (3) A
 * breakdown of omega in pass X: pass X wrote nothing, pass P publishes it.  A cycle never writes x, r, v, t, rhat or a scalar of the loop.
 * Refused with MGCG_ERROR, a message and nothing enqueued: everything SolveBicgstab refuses; a null mg; a hierarchy of several ranks; a
 * hierarchy whose level 0 does not have `count` rows ("... rows on level 0, the matrix has ...", as SolveMinresMg).
 * Out of scope: several ranks (SolveBicgstabMgParallel), changes inside the cycle's kernels, the C++ twin under host/. */
int SolveBicgstabMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                    Vector* vVector, Vector* sVector, Vector* tVector, Vector* rhatVector,
                    int elementsCount, int count,
                    double allowableResidual, int minIteration, int maxIteration, int rule,
                    int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- BiCGStab(l): nonsymmetric systems where BiCGStab's degree-1 steps break down, l = 1 .. 4, plain and Jacobi (one rank) ---- */
/* Sleijpen and Fokkema's BiCGStab(l).  SolveBicgstab's residual polynomial gains one real root per body (a degree-1 minimal-residual step); when
 * the spectrum of A lies near the imaginary axis (convection dominates) omega drifts to 0 and that loop stagnates or ends MGCG_NONFINITE.  Here
 * a body is l BiCG steps and ONE minimal-residual step of degree l over r_0 .. r_l, so the polynomial may have complex roots.  Same needs as
 * SolveBicgstab: products with A only, fixed storage, right-preconditioned with M = I (SolveBicgstabL) or M = diag(A) (SolveBicgstabLJacobi), so
 * r_0 stays the residual of the system itself and every stop rule judges its 2-norm.  A body costs 2 l products; one rank: 4 l + 2 launches.
 * The minimal-residual step is solved from the Gram matrix Z_ab = r_a.r_b (normal equations, Cholesky) and not by modified Gram-Schmidt: one
 * pass over r_0 .. r_l and one reduction point in place of l (l + 1) / 2 dependent ones.
 * Method: d_i is dinv_i when a diagonal is given and 1 otherwise; with d = 1 the multiplication is not performed and no hatted copy is stored.
 * hat(v)_i = d_i*v_i.  The vectors are r_0 .. r_l, u_0 .. u_l, the shadow rt, and x.
 *   start   (MGCG_RULE_SIMPLE: x := 0)
 *           r_0 = b - A x ;  rt = r_0 ;  u_0 = r_0 ;  rho = rr0 = r_0.r_0
 *           rr0 == 0 or not finite  ->  MGCG_NONFINITE at iteration 0, x untouched
 *   body k  for j = 0 .. l-1:
 *             j > 0:  rrj = r_0.r_0 ;  when the rule's stop test on (rrj, rr0) for iteration k + 1 says "converged", the body ends here:
 *                     iteration k + 1 with rrj as its figure, MGCG_OK (a cap that is exceeded or a value that is not finite waits for the
 *                     body's end)
 *                     rho1 = rt.r_j (the sum the product that made r_j left) ;  beta = alpha*(rho1/rho) ;  rho = rho1
 *                     u_i = r_i - beta*u_i,  i = 0 .. j                                                              (pass U_j)
 *             u_{j+1} = A hat(u_j) ;  sigma = rt.u_{j+1}
 *             sigma == 0 or not finite, or alpha = rho/sigma not finite  ->  MGCG_NONFINITE for iteration k + 1 ;  x and r_0 are what steps
 *                     0 .. j-1 of this body made them (a consistent pair)
 *             r_i = r_i - alpha*u_{i+1},  i = 0 .. j ;  x = x + alpha*hat(u_0)                                         (pass R_j)
 *             r_{j+1} = A hat(r_j) ;  the sum rt.r_{j+1}
 *           Z_ab = r_a.r_b,  a = 1 .. l,  b = 0 .. a                                                                   (Gram pass)
 *           gamma:  G = Z[1..l, 1..l].  Cholesky factor C, row by row: for i = 1 .. l { for j = 1 .. i-1 { s = G_ij ; for q = 1 .. j-1:
 *                     s = s - C_iq*C_jq ;  C_ij = s/C_jj }  s = G_ii ; for q = 1 .. i-1: s = s - C_iq*C_iq ;  pivot_i = s ;  C_ii = sqrt(s) }
 *                   m = the number of leading pivots that are > 0 and finite (the factorisation ends at the first that is not)
 *                   forwards:  for i = 1 .. m { s = Z_i0 ; for q = 1 .. i-1: s = s - C_iq*y_q ;  y_i = s/C_ii }
 *                   backwards: for i = m .. 1 { s = y_i ; for q = i+1 .. m: s = s - C_qi*gamma_q ;  gamma_i = s/C_ii }
 *                   gamma_{m+1 .. l} = 0 ;  omega = gamma_l
 *           u_0 = u_0 - gamma_j*u_j ;  x = x + gamma_j*hat(r_{j-1}) ;  r_0 = r_0 - gamma_j*r_j,  each for j = 1, 2 .. l in that order, one
 *                   term at a time (all l terms, those with gamma_j = 0 included; the r_0 of x's first term is the one the steps left) ;
 *                   rr = r_0.r_0 ;  rhon = rt.r_0                                                                      (combine pass)
 *           rr is judged by the rule's stop test against rr0 as the residual of iteration k + 1
 *           not stopped and (omega == 0 or rhon == 0 or rhon not finite)  ->  MGCG_NONFINITE for iteration k + 1 (x IS this body's iterate)
 *           beta = alpha*(rhon/((-omega)*rho)) ;  rho = rhon ;  u_0 = r_0 - beta*u_0                                   (pass P)
 *   end     one more product: rVector = b - A x ;  *trueResidual = sqrt(r.r)      (whenever the loop ended without MGCG_ERROR)
 * With l = 1 this is BiCGStab in other words (omega = Z_10 / Z_11 through a square root and two divisions), not bit for bit SolveBicgstab.
 * Rounding contract, SolveBicgstab's: every product (beta*u_i, alpha*u_{i+1}, d_i*u_0_i, alpha*hat(u_0)_i, C_iq*C_jq, C_iq*y_q, C_qi*gamma_q,
 * gamma_j*u_j, d_i*r_{j-1}_i, gamma_j*hat(r_{j-1})_i, gamma_j*r_j, and the terms of every sum) goes into a double of its own before the add or
 * subtraction that follows it, nothing is fused; the scalars are evaluated in exactly the order written (rho1/rho first, then times alpha;
 * -omega, times rho, rhon over that, times alpha).  Under dot_order = 1 every sum is serial left to right: the whole loop is then a fixed
 * sequence of IEEE operations (tests/test_bicgstabl_host.py restates it in numpy).
 * `iteration`, minIteration, maxIteration and the trace count BODIES; a body is 2 l products.  Stop: the four 2-norm rules of SolveEx on
 * (rr, rr0); MGCG_RULE_HANDMADECL is refused.  *iteration, *residual and the trace show the recurrence's figure as in SolveBicgstab; a
 * breakdown repeats the last judged figure.  WHY THE TEST IN FRONT OF A STEP.  When the Krylov space is exhausted inside a body (fewer rows
 * than l, a right-hand side made of few eigenvectors) r_0 is at rounding level and the steps behind it are quotients of rounding errors: on
 * the 2 x 2 matrix [[2, -.5], [-1.5, 2]] with l = 3, step 2 has rho = 6.7e-16, sigma = 6.9e-31 and alpha = 9.7e14, and moves x by 1e-2 while
 * the recurrence's r_0 stays at 1e-16 -- MGCG_OK with a true residual of 8e-2.  Judging r_0 in front of steps 1 .. l-1 costs no read (pass
 * R_j sums the r_0 it writes) and ends such a body where it converged; the last body of a run may so have fewer than 2 l products.  The
 * truncated factorisation does the same for the minimal-residual step: trailing pivots that are 0, negative or not finite are dropped.
 *   rVector         r_0 (count entries).  On return its first count entries hold the true residual b - A x
 *   pVector         u_0 (count entries)
 *   ApVector        u_l (count entries)
 *   workVector      slices of `count` entries, count rounded up to even apart (every slice stays 16-byte aligned): r_1 .. r_l, then
 *                   u_1 .. u_{l-1}, then rt, and in the Jacobi form the one gather buffer that holds hat(u_j) or hat(r_j) for the next
 *                   product -- 2 l slices, 2 l + 1 with a diagonal.  Without a diagonal the products gather from u_j and r_j themselves.
 * Refused with MGCG_ERROR, a message and nothing enqueued: ell outside 1 .. 4 ("ell = 5, must be 1 .. 4"), a work vector that is too short
 * (with both sizes), MGCG_RULE_HANDMADECL, and everything SolveBicgstab refuses.
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update, the placement draw and the
 * overlap schedule do not apply.  GMRES: SolveGmres below.  Out of scope, and next: several ranks (SolveBicgstabLParallel), the V-cycle
 * form, l > 4, residual replacement, the C++ twin under host/. */
int SolveBicgstabL(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                   Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
                   int ell, int elementsCount, int count,
                   double allowableResidual, int minIteration, int maxIteration, int rule,
                   int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
int SolveBicgstabLJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                         Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                         Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector, Vector* dinvVector,
                         int ell, int elementsCount, int count,
                         double allowableResidual, int minIteration, int maxIteration, int rule,
                         int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- Restarted GMRES(m): the nonsymmetric solver whose residual never increases, 1 <= m <= 32, plain and Jacobi (one rank) ---- */
/* Saad and Schultz's GMRES, restarted every m steps.  Against SolveBicgstab and SolveBicgstabL it has three properties: the judged residual
 * never increases (theirs can peak many orders above || b ||), it cannot break down on a nonsingular matrix (they end MGCG_NONFINITE where
 * convection dominates), and it does not drift -- every restart recomputes r = b - A x by a product.  It pays with storage (m + 1 vectors)
 * and traffic (a step touches every column of the cycle): slower per product than both, see DESIGN.md.  Same needs otherwise: products with
 * A only, right-preconditioned with M = I (SolveGmres) or M = diag(A) (SolveGmresJacobi), so the judged residual is that of A x = b in the
 * 2-norm.  The orthogonalisation is CLASSICAL Gram-Schmidt applied `orth` times (1 or 2; 2 is "twice is enough"), not modified Gram-Schmidt:
 * the j + 1 sums of a pass are independent and share one reduction point, where the modified form needs j + 1 dependent ones.
 * Method: d_i is dinv_i when a diagonal is given and 1 otherwise; with d = 1 the multiplication is not performed and no hatted copy is stored.
 * hat(v)_i = d_i*v_i.  An ITERATION is one Arnoldi step, which is one product; k counts them from 0, j = k mod m is the step's place in its cycle.
 *   start   (MGCG_RULE_SIMPLE: x := 0)
 *           r = b - A x ;  beta2 = rr0 = r.r ;  rr0 == 0 or not finite  ->  MGCG_NONFINITE at iteration 0, x untouched
 *           beta = sqrt(beta2) ;  v_0 = r/beta ;  g_0 = beta
 *   step k  w = A hat(v_j)
 *           `orth` times:  h'_i = v_i.w,  i = 0 .. j ;  w = w - h'_i*v_i  for i = 0, 1 .. j in that order, one term at a time ;
 *                          the first time h_i = h'_i, the second time h_i = h_i + h'_i
 *           hn2 = w.w ;  hn = sqrt(hn2)                                                                                (pass N)
 *           for i = 0 .. j-1:  t1 = c_i*h_i ; t2 = s_i*h_{i+1} ; t3 = s_i*h_i ; t4 = c_i*h_{i+1} ;  h_i = t1 + t2 ;  h_{i+1} = t4 - t3
 *           d = sqrt(h_j*h_j + hn*hn)     (two products, an add, a square root: no hypot)
 *           hn2 not finite, or d == 0 or not finite  ->  MGCG_NONFINITE for iteration k + 1 with the last judged figure once more; this
 *                   step adds no column (A is singular on the Krylov space, or a value is not finite)
 *           c_j = h_j/d ;  s_j = hn/d ;  g_{j+1} = (-s_j)*g_j ;  g_j = c_j*g_j ;  R_ij = h_i (i < j) ;  R_jj = d ;  the cycle has j + 1 columns
 *           g_{j+1}*g_{j+1} is judged by the rule's stop test against rr0 as the squared residual of iteration k + 1
 *           hn2 == 0  ->  the Krylov space is exhausted: MGCG_OK at iteration k + 1 with residual 0, whatever minIteration says
 *           not stopped:  v_{j+1} = w/hn
 *   close   once per cycle -- behind step j = m - 1, and for the cycle cut short by a stop, the cap or a breakdown -- over its `cols` columns:
 *           for i = cols-1 .. 0 { s = g_i ; for q = i+1 .. cols-1: s = s - R_iq*y_q ;  y_i = s/R_ii }
 *           in groups of 8 columns, c0 = 0, 8 ..:  t = 0 ; for i = c0 .. min(c0 + 8, cols) - 1: t = t + y_i*v_i ;  x = x + hat(t)
 *   restart r = b - A x ;  beta2 = r.r ;  judges nothing, but beta2 == 0  ->  MGCG_OK at iteration k with residual 0 (no trace entry), and
 *           beta2 not finite  ->  MGCG_NONFINITE at iteration k with the last judged figure ;  else beta, v_0, g_0 as at the start
 *   end     one more product: rVector = b - A x ;  *trueResidual = sqrt(r.r)      (whenever the loop ended without MGCG_ERROR)
 * Rounding contract, SolveBicgstab's: every product (h'_i*v_i, the t's of a rotation, h_j*h_j, hn*hn, (-s_j)*g_j, c_j*g_j, R_iq*y_q,
 * y_i*v_i, d_i*t_i, and the terms of every sum) goes into a double of its own before the add or subtraction that follows it, nothing is
 * fused; v_0 and v_{j+1} are formed by division.  Under dot_order = 1 every sum is serial left to right: the whole loop is then a fixed
 * sequence of IEEE operations (tests/test_gmres_host.py restates it in numpy).
 * `iteration`, minIteration, maxIteration and the trace count STEPS: trace[0] is the first residual, trace[k] the figure after step k.  Stop:
 * the four 2-norm rules of SolveEx on (g_{j+1}^2, rr0); MGCG_RULE_HANDMADECL is refused.  *iteration, *residual and the trace show the rotated
 * estimate |g_{j+1}|, which a restart replaces by the explicit || b - A x ||.
 *   rVector         b - A x of the start and of every restart (count entries).  On return its first count entries hold the true residual
 *   pVector         the buffer the residual products gather x from (count entries)
 *   ApVector        w (count entries)
 *   workVector      slices of `count` entries, count rounded up to even apart (every slice stays 16-byte aligned): v_0 .. v_m, and in the
 *                   Jacobi form the one gather buffer that holds hat(v_j) for the next product -- m + 1 slices, m + 2 with a diagonal.
 *                   Whatever it holds on entry does not reach the result.
 * Refused with MGCG_ERROR, a message and nothing enqueued: m outside 1 .. 32 ("m = 33, must be 1 .. 32"), orth outside {1, 2}, a work vector
 * that is too short (with both sizes), MGCG_RULE_HANDMADECL, and everything SolveBicgstab refuses; a communicator of several ranks ("the loop
 * runs on one rank").
 * The matrix product is SolveEx's (compression modes and the automatic column tiles apply); the deferred x update, the placement draw and the
 * overlap schedule do not apply.  The V-cycle as preconditioner, in the flexible form: SolveGmresMg below.  Out of scope, and next: several
 * ranks, a non-flexible V-cycle form, m > 32, the C++ twin under host/, the front-ends. */
int SolveGmres(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
               int m, int orth, int elementsCount, int count,
               double allowableResidual, int minIteration, int maxIteration, int rule,
               int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);
int SolveGmresJacobi(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                     Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                     Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector, Vector* dinvVector,
                     int m, int orth, int elementsCount, int count,
                     double allowableResidual, int minIteration, int maxIteration, int rule,
                     int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- V-cycle-preconditioned flexible GMRES(m): the robust nonsymmetric solver with this library's strongest preconditioner (one rank) ---- */
/* SolveGmres right-preconditioned with the V-cycle of a hierarchy (MgSetup, MgSetupAggregation, MgSetupAggregates; either smoother), in Saad's
 * FLEXIBLE form: z_j = M^-1 v_j is stored beside the basis and the close adds sum y_i z_i.  SolveBicgstabMg is the faster loop where it
 * converges; where convection dominates (a central stencil at cell Peclet number >= 2) it ends MGCG_NONFINITE and this loop still converges --
 * slowly: there the Jacobi-smoothed cycle is a poor map, and what is bought is robustness, not speed.  As in
 * SolveBicgstabMg the hierarchy may come from ANY matrix with `count` rows, the matrix itself or its symmetric part, for instance; only its
 * row count is checked.  The flexible form asks nothing of M, not even that it be a fixed linear map.
 * Method: SolveGmres's with d = 1, line by line, and these changes only.
 *   start   as SolveGmres
 *   step k  z_j = M^-1 v_j            MgApply's fixed sequence of operations on the caller's hierarchy, written straight into slice z_j
 *           w = A z_j                 the product gathers from that slice
 *           the `orth` Gram-Schmidt passes over v_0 .. v_j, pass N, the rotations, both no-next-direction branches, the stop decision,
 *           the trace, the iteration count and v_{j+1} = w/hn: SolveGmres's, unchanged, on V
 *   close   y as in SolveGmres ;  in groups of 8 columns, c0 = 0, 8 ..:  t = 0 ; for i = c0 .. min(c0 + 8, cols) - 1: t = t + y_i*z_i ;
 *           x = x + t                 (SolveGmres's close with Z in place of V: same groups, term order and rounding contract)
 *   restart, end   as SolveGmres
 * A cycle runs after the start, after every restart and after every pass N that did not stop: in front of every product, m per cycle of m
 * steps and none in the close (x = x + M^-1 (V y) would need one there).  The judged figure is the 2-norm of the system's own residual (right
 * preconditioning); minIteration, maxIteration, the trace and *iteration count steps of one cycle and one product each.  Under dot_order = 1
 * the whole loop is a fixed sequence of IEEE operations (tests/test_gmres_mg_host.py restates it in numpy with Hierarchy.apply).
 * FLAG DISCIPLINE.  The cycle and the product take the LIVE stop flag as their gate: pass N alone raises it, and no workgroup of pass N runs
 * beside them (one stream).  A cycle enqueued behind a stop therefore returns at the gate in every one of its kernels and leaves z_{j+1}
 * unwritten; the close reads columns i < cols only, and column cols - 1 = j was written by the cycle in front of step j, which ran with the
 * flag down -- so an unwritten slice is never read, and a work vector full of NaN on entry does not reach the result.  A cycle writes its z
 * slice and the hierarchy's own iterates, never x, V, w or a scalar of the loop.  The close launches stay ungated and keyed on cols / yCount,
 * as in SolveGmres: x is updated exactly once per cycle whatever was enqueued behind the stop.  A restart that found r.r zero or not finite
 * wrote no v_0; the cycle and the product behind it run on the previous cycle's v_0 and write z_0 and w only, which nothing reads: the next
 * pass N publishes the end and cols is 0.
 *   workVector      slices of `count` entries, count rounded up to even apart: v_0 .. v_m, then z_0 .. z_{m-1} -- 2 m + 1 slices (41 vectors
 *                   at m = 20).  Whatever it holds on entry does not reach the result.
 *   rVector, pVector, ApVector   as SolveGmres
 * Refused with MGCG_ERROR, a message and nothing enqueued: everything SolveGmres refuses (m outside 1 .. 32, orth outside {1, 2}, the rule,
 * a communicator of several ranks); a work vector shorter than 2 m + 1 slices (with both sizes); a null mg; a hierarchy of several ranks; a
 * hierarchy whose level 0 does not have `count` rows ("... rows on level 0, the matrix has ...", as SolveMinresMg).
 * Out of scope, and next: several ranks, a non-flexible form (x = x + M^-1 (V y): m fewer slices, one more cycle per restart, and a gated
 * cycle inside the ungated close), m > 32, changes inside the cycle's kernels, the C++ twin under host/. */
int SolveGmresMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* workVector,
                 int m, int orth, int elementsCount, int count,
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int* iteration, double* residual, double* trueResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- LSQR: least squares min || A x - b ||_2 for a rectangular CSR matrix, optionally damped (one rank) ---- */
/* Paige and Saunders' LSQR.  A is any CSR matrix of rows x columns -- more rows than columns or fewer, square and nonsymmetric, rank
 * deficient -- and b any right-hand side, consistent or not.  The call minimises || A x - b ||^2 + damp^2 || x ||^2 (damp >= 0; 0: plain least
 * squares) and, where the minimiser is not unique, tends to the one of minimum norm.  It is analytically CG on the normal equations
 * (A^T A + damp^2 I) x = A^T b without ever forming A^T A; it converges on that spectrum, so on a square system that BiCGStab or GMRES solve
 * it is the slower method, and it is the one that still works where those are undefined.
 * The caller hands in TWO CSR triples: A, and A^T (columns x rows) exactly as MgcgCsrTranspose writes it.  THE LIBRARY DOES NOT VERIFY THAT
 * THE SECOND IS THE TRANSPOSE OF THE FIRST.  The transposed product is therefore the ordinary gather product on A^T: deterministic, no
 * float atomics, row c of A^T summed in ascending stored position of A.  Both products are CsrMV's (rectangular operands; compression modes
 * and the automatic column tiles apply to each matrix by itself).
 * Method (the bidiagonalisation u_k, v_k with || u || = || v || = 1; lambda = damp):
 *   start   x := 0 under EVERY rule (the caller's x is overwritten: callers with a guess x0 pass b - A x0 and add x0 back)
 *           beta_1 = || b || ; u_1 = b/beta_1 ; alpha_1 = || A^T u_1 || ; v_1 = A^T u_1/alpha_1 ; w_1 = v_1 ; phibar_1 = beta_1 ; rhobar_1 = alpha_1 ;
 *           g_0 = alpha_1 beta_1 ; Psi = 0
 *   body k  beta_k+1 u_k+1 = A v_k - alpha_k u_k ;  alpha_k+1 v_k+1 = A^T u_k+1 - beta_k+1 v_k
 *           damp != 0: rhobar' = sqrt(rhobar^2 + lambda^2) ; psi = (lambda/rhobar') phibar ; phibar = (rhobar/rhobar') phibar ; Psi += psi^2 ; rhobar = rhobar'
 *           rho = sqrt(rhobar^2 + beta_k+1^2) ; c = rhobar/rho ; s = beta_k+1/rho ; theta = s alpha_k+1 ; rhobar = -c alpha_k+1 ; phi = c phibar ; phibar = s phibar
 *           x += (phi/rho) w ;  w = v_k+1 - (theta/rho) w
 *           judged: g = |phibar| alpha_k+1 |c|, the estimate of || A^T (b - A x) - lambda^2 x ||_2 ; kept: sqrt(phibar^2 + Psi), the estimate of
 *           the (damped) residual norm
 * As computed -- the vectors stay UNNORMALISED in memory, uh = beta u (rows) and vh = alpha v (columns), and the w update of body k is done
 * by body k + 1 (its theta needs alpha_k+1, which is known only behind the pass that writes x); k counts from 0 here:
 *   start   x = 0 ; uh = b ; bb = b.b ; beta = sqrt(bb) ; t = A^T uh ; vh_j = t_j*(1/beta) ; vv = vh.vh ; alpha = sqrt(vv) ; g0 = alpha*beta ;
 *           gg0 = g0*g0 ; phibar = beta ; rhobar = alpha ; Psi = 0 ; trace[0] = g0 (sqrt(gg0/gg0) under MGCG_RULE_VIENNACL)
 *           bb zero or not finite  ->  MGCG_NONFINITE at iteration 0 with g0 := beta ; else vv, else gg0 zero or not finite  ->  the same (the
 *           message says which: "beta_1 = || b ||", "alpha_1 = || A^T b || / beta_1", "g_0")
 *   body k  q = A vh
 *   pass U  ia = 1/alpha ; ab = alpha/beta ;  uh_i = q_i*ia - ab*uh_i ;  uu = uh.uh                                            (24 bytes per row)
 *   t = A^T uh
 *   pass V  betan = sqrt(uu)
 *           damp != 0: rd = sqrt(rhobar*rhobar + damp*damp) ; psi = (damp/rd)*phibar ; phibar = (rhobar/rd)*phibar ; Psi = Psi + psi*psi ; rhobar = rd
 *           rho = sqrt(rhobar*rhobar + betan*betan) ; c = rhobar/rho ; s = betan/rho ; phi = c*phibar ; phibarn = s*phibar ; xs = phi/rho
 *           betan, rho, xs, phibarn or Psi not finite, or rho == 0  ->  MGCG_NONFINITE reported for iteration k + 1, nothing changed by this body
 *           vn_j = vh_j*ia ;  w_j = vn_j - tr*w_j  (k = 0: w_j = vn_j, w is not read) ;  x_j = x_j + xs*w_j
 *           vh_j = t_j*(1/betan) - betan*vn_j ;  vv = vh.vh        (betan == 0: vh is not formed)                         (56 bytes per column)
 *   scalars alphan = sqrt(vv) (0 when betan == 0) ; theta = s*alphan ; rhobar = -(c*alphan) ; tr = theta/rho ; g = (|phibarn|*alphan)*|c| ;
 *           gg = g*g ; the estimate sqrt(phibarn*phibarn + Psi) ; gg is judged by the rule's stop test against gg0 as iteration k + 1
 *           g == 0 (betan or alphan exactly zero): x is the solution -- the loop ends here with MGCG_OK, whatever minIteration says
 *           alphan or g not finite  ->  MGCG_NONFINITE for iteration k + 1; x is this body's, every scalar of whose update was finite
 *           alpha = alphan ; beta = betan ; phibar = phibarn
 *   end     two closing products, whenever the loop ended without MGCG_ERROR: uVector = b - A x ; tVector = A^T uVector, and with damp != 0
 *           t_j = t_j - (damp*damp)*x_j ;  *trueResidual = sqrt(u.u) ;  *trueNormalResidual = sqrt(t.t)
 * Rounding contract: every product and every quotient goes into a double of its own before the add or subtraction that follows it, nothing
 * is fused; 1/alpha, 1/beta, 1/betan, alpha/beta and phi/rho are formed once and multiplied; every square root is sqrt of two separately
 * rounded squares and their sum, never hypot; a matrix row is summed as CsrMV sums it; the terms of the sums are b_i*b_i, vh_j*vh_j, uh_i*uh_i,
 * u_i*u_i and t_j*t_j of the rounded values.  Under dot_order = 1 every sum is serial left to right and the whole loop is a fixed sequence of
 * IEEE operations (tests/test_lsqr_host.py restates it in numpy).
 * Stop: the four 2-norm rules of SolveEx on (gg, gg0), exactly as SolveMinres applies them to (rr, rr0); MGCG_RULE_HANDMADECL is refused.
 * g is judged because it tends to zero for consistent and inconsistent systems alike; || b - A x || does not.  *iteration, *residual and the
 * trace show sqrt(gg) (g itself unless g*g underflows; sqrt(gg/gg0) in the trace under MGCG_RULE_VIENNACL); *residualNorm (may be NULL) the
 * estimate of the residual norm at the last judged body (beta_1 at iteration 0); *trueResidual and *trueNormalResidual (may be NULL) the
 * closing products' figures.  A breakdown repeats the last judged figure in *residual and its trace entry.
 * One body is five launches with two reduction points: the two products, the two passes above and one single-workgroup launch for the
 * scalars behind pass V.  Vector traffic per body: 24 bytes per row + 56 per column, next to the two products (each reads its matrix once,
 * gathers one vector and writes the other).
 *   xVector (columns)  the result; bVector (rows) is only read
 *   uVector (rows)     uh during the loop; on return b - A x
 *   tVector (columns)  A^T uh during the loop; on return A^T (b - A x) - damp^2 x
 *   vVector, wVector (columns), qVector (rows)   work space: vh, w, q.  No work vector and no x is read before the call has written it.
 * Refused with MGCG_ERROR, a message and nothing enqueued, before a device is asked for: a null handle; rows < 1, columns < 1 or
 * elementsCount < 0 ("bad sizes"); a vector of A or of A^T smaller than elementsCount / rows + 1 / columns + 1; a vector too small for its role
 * ("the x vector holds .. entries, the matrix has .. columns": x, v, w, t by columns; b, u, q by rows); damp negative or not finite; an unknown
 * rule or MGCG_RULE_HANDMADECL.
 * Out of scope: several ranks (a row partition of A makes A^T u a sum across ranks), preconditioning, LSMR, an initial guess, fusing the
 * passes into the products' epilogues, the C++ twin under host/. */
int MgcgSolveLsqr(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
              Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,        /* A: rows x columns */
              Vector* elementsTVector, VectorInt* rowOffsetsTVector, VectorInt* columnIndecesTVector,     /* A^T: columns x rows (MgcgCsrTranspose) */
              Vector* xVector, Vector* bVector, Vector* uVector, Vector* vVector, Vector* wVector, Vector* qVector, Vector* tVector,
              int elementsCount, int rows, int columns, double damp,
              double allowableResidual, int minIteration, int maxIteration, int rule,
              int* iteration, double* residual, double* residualNorm /* may be NULL */, double* trueResidual /* may be NULL */,
              double* trueNormalResidual /* may be NULL */, double* residualTrace, int traceCapacity);

/* ---- LOBPCG: the k extreme eigenpairs of a symmetric CSR matrix (one rank) ---- */
/* MgcgSolveLobpcg: Knyazev's locally optimal block preconditioned CG for the k = 1 .. 8 lowest eigenpairs A x_j = theta_j x_j of a symmetric
 * count x count CSR matrix (symmetry is not checked), fp64, the matrix read as plain CSR by CsrMVBlock's k-column product whatever
 * compression mode the handle carries.  "Lowest" means highest when largest = 1.  xVector holds the n x k start block X on entry and the
 * eigenvectors on return, column j at [j*count, (j+1)*count) as CsrMVBlock takes it.  The preconditioner M^-1 is the identity, the diagonal's
 * inverse (dinvVector: what MgcgJacobiSetup wrote) or, in MgcgSolveLobpcgMg, the cycle of a one-rank hierarchy whose level 0 has count rows
 * (MgSetup, MgSetupAggregation(Ex), MgSetupAggregates, the Gauss-Seidel / SSOR and the ILU(0) handles; k calls of MgApply's cycle per body).
 * The method as computed (m = 3k columns, 2k while P is absent):
 *   start   AX = A X ;  G = X^T X = U^T U (Cholesky, U upper) ;  X = X U^-1 ; AX = AX U^-1
 *           H = X^T AX (upper triangle, mirrored) = Z diag(theta) Z^T (cyclic Jacobi, below) ;  X = X Z ; AX = AX Z ;  P absent
 *   body i  R = AX - X diag(theta) ;  rn_j = || R_j ||_2 ;  the stop decision (below)
 *           W_j = M^-1 R_j  (identity: W = R; dinv: W = dinv o R inside the same pass; hierarchy: k cycles on the columns)
 *           T = X^T W (all k x k entries) ;  W_j = W_j - sum_l X_l T[l][j]
 *           G = W^T W ;  d_a = 1 / sqrt(G_aa) (a G_aa that is not finite and > 0 -- a zero column of W -- : breakdown "W", pivot a) ;
 *           (d_a G_ab) d_b = U^T U (a failed pivot: breakdown "W") ;  W = W (D U^-1): the columns scaled to 2-norm 1 and orthonormalised,
 *           both through one k x k coefficient block D U^-1 with (D U^-1)[l][j] = d_l U^-1[l][j]
 *           AW = A W                                       (the one k-column product of the body)
 *           S = [X W P], AS = [AX AW AP] ;  G_B = S^T S , G_A = S^T AS   (upper triangles, all entries summed: none is assumed 0 or 1)
 *           G_B = U^T U ;  with P present a pivot d_i must be finite, > 0 and > 2^-20 (G_B)_ii (computed as d_i > 2^-20 * (G_B)_ii): else P
 *                          is dropped for this body and the next and the leading 2k problem is formed instead (counted in *restarts);
 *                          with P absent the test is the raw one, finite and > 0, and a failure is breakdown "basis".  (The error of H
 *                          is about eps / min d_i: a basis that passes only the raw test lets columns that converged long ago drift
 *                          until the loop breaks down -- poisson(7,6,5), k = 5, Jacobi: NONFINITE in body 105; it converges with the
 *                          floor, which keeps that error below 2^-33.)
 *           H = U^-T (G_A U^-1) (G_A mirrored, both products with full sums; H's upper triangle mirrored) ;  H = Z diag(w) Z^T ;
 *           C = U^-1 Z[:, lowest k] ;  theta = those w, ascending (descending for largest) ;  a theta that is not finite: breakdown
 *           Pnew = [W P] C[k:, :] scaled by 1 / sqrt(c_j^T G_B[k:, k:] c_j), its column's 2-norm out of the Gram matrix (c_j = C[k:, j];
 *           G_B[k:, k:] c_j first, then the sum over its rows; a value that is not finite and > 0 gives the factor 0), APnew by the same
 *           factor ;  X = S C ;  AX = AS C ;  P = Pnew ; AP = APnew       (one row-local pass, in place)
 *   close   AX = A X by one more product ;  trueResidual_j = || AX_j - theta_j X_j ||_2 ;  the work vector's R block holds those columns
 * Nothing is frozen: every column is updated until the loop ends.
 * The dense symmetric eigenproblem H = Z diag(w) Z^T (order at most 24) is solved by cyclic Jacobi rotations on the device: Z = I; a sweep
 * visits (p, q) for p = 0 .. m-2, q = p+1 .. m-1 in that order; a pair with |h_pq| <= 2^-53 (|h_pp| + |h_qq|) (or a NaN there) is passed over;
 * otherwise tau = (h_qq - h_pp) / (2 h_pq), t = 1 / (|tau| + sqrt(1 + tau*tau)) with the sign of tau (+ for 0), c = 1 / sqrt(1 + t*t),
 * s = t c; for every r but p and q: h_rp = h_pr = c h_rp - s h_rq and h_rq = h_qr = s h_rp + c h_rq (of the old values);
 * h_pp = h_pp - t h_pq, h_qq = h_qq + t h_pq (old h_pq), h_pq = h_qp = 0; for every r: z_rp = c z_rp - s z_rq, z_rq = s z_rp + c z_rq.
 * The sweeps end behind the first sweep that rotated nothing, or behind 30.  w is the diagonal; it is sorted ascending (descending for
 * largest) by a stable sort: equal values keep their index order.
 * Stop: column j is converged when rn_j <= allowableResidual (relative = 0) or rn_j <= allowableResidual |theta_j| (relative = 1).  The
 * loop ends in the first body i in which every column is converged and i >= minIteration (MGCG_OK), else in body i >= maxIteration
 * (MGCG_MAXIT_EXCEEDED; status[j] then says which columns had converged).  The decision is made on the device; the host looks at the flag
 * every check_every bodies.  *iteration is the index of the last body that was judged; residual[j] = rn_j, theta[j], status[j] and the trace
 * (rn_j of body i at residualTrace[j*traceCapacity + i], the first min(*iteration + 1, traceCapacity) entries) belong to that body.
 * Breakdown: a failed first factorisation (dependent or zero start columns, a value that is not finite), a failure in "W" or "basis", or a
 * theta that is not finite ends the call with MGCG_NONFINITE for every column; X, AX and theta of the last completed body are kept (a valid
 * orthonormal Ritz block; after a failed start no body was judged: *iteration is -1 and trueResidual NaN; X is the caller's after a failed
 * first factorisation and X U^-1, orthonormal, where a Ritz value of the start block is not finite); MgcgGetLastError names the factorisation and the pivot.
 * Rounding contract: every product goes into a double of its own before the add or subtraction that follows it, nothing is fused; a sum over
 * a block index starts with its first product and adds the others left to right, structural zeros included; the Cholesky factorisation and
 * the triangular inverse are SolveBlockKrylov's; a Gram entry sum_i a_i b_i is a fixed tree of per-workgroup partial sums, and one serial
 * left-to-right sum over the rows under dot_order = 1, which makes the whole loop a fixed sequence of IEEE operations
 * (tests/test_lobpcg_host.py restates it in numpy).
 *   workVector  MgcgLobpcgWorkSize(count, k) entries: the six blocks AX, W, AW, P, AP, R of k columns each, every column count rounded up
 *               to even apart: a 64-bit count, as the sizes of the vectors are (512^3 rows with k = 4 need 3.2e9).  0 from
 *               MgcgLobpcgWorkSize means bad sizes (count < 1 or k outside 1 .. 8); no call is accepted with a work vector of fewer entries.
 * Refused with MGCG_ERROR, a message and nothing enqueued, before a device is asked for: a null handle; k outside 1 .. 8; count < 1 or
 * elementsCount < 0; 3k > count; largest or relative outside {0, 1}; allowableResidual negative or not finite; largest = 1 with a hierarchy;
 * a vector of the matrix, x (k count entries), the work vector or dinv too small, each named; a hierarchy of several ranks or whose level 0
 * has not count rows.
 * Out of scope: soft locking of converged columns, generalised problems A x = lambda B x, k > 8, several ranks, interior eigenvalues and
 * shift-invert, the C++ twin under host/; MgcgEstimateSpectrum stays as it is. */
long long MgcgLobpcgWorkSize(int count, int k);
int MgcgSolveLobpcg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                    Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                    Vector* xVector /* count*k, in: start block, out: eigenvectors */, Vector* workVector, Vector* dinvVector /* may be NULL */,
                    int elementsCount, int count, int k, int largest,
                    double allowableResidual, int relative, int minIteration, int maxIteration,
                    int* iteration, double theta[], double residual[], double trueResidual[] /* may be NULL */, int status[], int* restarts,
                    double residualTrace[], int traceCapacity);
int MgcgSolveLobpcgMg(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr, MgcgMg* mg,
                      Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                      Vector* xVector, Vector* workVector,
                      int elementsCount, int count, int k, int largest,
                      double allowableResidual, int relative, int minIteration, int maxIteration,
                      int* iteration, double theta[], double residual[], double trueResidual[] /* may be NULL */, int status[], int* restarts,
                      double residualTrace[], int traceCapacity);

/* ---- Chebyshev-preconditioned CG: a polynomial preconditioner for any CSR matrix, no global sum inside it (one rank or several) ---- */
/* *bound = the maximum, over the local rows [offsetForDevice, +countForDevice), of sum_j |a_ij| -- times dinv_i when dinvVector (what
 * MgcgJacobiSetup wrote) is given: Gershgorin's upper bound of the spectrum of A (of D^-1 A), rigorous, usually within a small factor
 * of lambda_max for diagonally dominant matrices.  Each row is summed in stored order from +0.0 on the device; one read-back.  An
 * empty local slice gives 0; several ranks take the maximum of their bounds themselves.  Returns 0 on success, -1 with a message. */
int MgcgGershgorinBound(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                        int elementsCount, int countForDevice, int offsetForDevice, Vector* dinvVector /* may be NULL */, double* bound);
/* SolveJacobi's loop with z = M r, M = p_m(B) D^-1 the Chebyshev polynomial of degree m - 1 in B = D^-1 A for the interval
 * [lambdaMin, lambdaMax] (D = I, B = A when dinvVector is NULL).  One iteration carries m products and still two global sums: the
 * polynomial needs no sum at all, and one of its steps is ONE launch (the product with the step fused into its epilogue).  One rank:
 * m + 3 launches per iteration (product, first pass, m - 1 steps, finalisation, x / p update).
 * Bounds and coefficients: 0 < lambdaMin < lambdaMax, both finite; degree m = 1 .. 16.  The host computes, once per call, in double
 * precision and in exactly this order
 *   theta = (lmax + lmin) * 0.5 ; delta = (lmax - lmin) * 0.5 ; sigma = theta / delta ; rho_0 = 1 / sigma ; it = 1 / theta
 *   j = 1 .. m-1:  rho_j = 1 / (2*sigma - rho_{j-1}) ; c1_j = rho_j * rho_{j-1} ; c2_j = (2 * rho_j) / delta
 * and hands the coefficients to the kernels as arguments.
 * Applying z = M r (every product is rounded into a double of its own before the add that follows it, nothing is fused):
 *   first   u_i = dinv_i * r_i (u_i = r_i without dinv) ; d_i = it * u_i ; z_i = d_i
 *   step j  acc_i = row i of A z, summed in stored order from +0.0 ; res = r_i - acc_i ; t = dinv_i * res (t = res without dinv)
 *           a = c1_j * d_i ; b = c2_j * t ; d_i = a + b ; z'_i = z_i + d_i          (z' is another buffer than z: rows gather z)
 *   the terms of r.z are r_i * z_i of the last z.
 * The outer loop: alpha = r.z / p.Ap ; r = r + (-alpha) Ap ; beta = r.z_new / r.z ; p = z + beta p ; x += alpha p, with SolveJacobi's
 * rounding.  The stop rules, the trace, *iteration and *residual are SolveJacobi's and test the TRUE residual; MGCG_RULE_HANDMADECL is
 * refused with MGCG_ERROR before anything is enqueued.  Under dot_order = 1 every sum is serial left to right and ranks add in rank order.
 * With m = 1 and bounds that make theta exactly 1.0 (0.5 and 1.5, say) z is D^-1 r bit for bit and the call returns SolveJacobi's x,
 * trace, iteration and residual exactly.
 * Breakdown: a p.Ap or an r.z that is not finite and > 0 ends the loop with MGCG_NONFINITE before that iteration's updates.  x keeps
 * the last completed iterate -- at the start the caller's x bit for bit (MGCG_RULE_SIMPLE: zero) -- *iteration is the iteration that
 * could not run, and *residual and its trace entry repeat the last judged residual.  The r.z of iteration k + 1 is formed at the end of
 * iteration k, behind k's stop test: when it breaks down, iteration k is complete (its x term applied, rVector its residual) and the
 * call reports iteration k + 1.  An upper bound BELOW the true lambda_max can make M indefinite, and a negative r.z is how that shows:
 * put a margin on an estimate that approaches lambda_max from below (a Lanczos value), or use MgcgGershgorinBound.  A lambdaMin above
 * the true lambda_min only costs iterations.  b = 0 from x = 0 gives r.z = 0 and MGCG_NONFINITE at iteration 0.
 *   dinvVector      what MgcgJacobiSetup wrote, or NULL; with it the bounds are bounds of D^-1 A
 *   zVector, z2Vector, dVector   work space with an internal layout (count entries each)
 * The steps always read the matrix as plain CSR, whatever the handle's compression mode (the lossless forms give the same bits); the
 * loop's own product p -> Ap is SolveEx's, so compression modes and the automatic column tiles apply to it.  The deferred x update
 * (x_defer) and the placement draw do not apply.  Out of scope: the step in the column-tile and propagation-blocking forms, the
 * V-cycle or the single-reduction loop combined with the polynomial, the block, shifted and mixed variants. */
int SolveChebyshev(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                   Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector /* may be NULL */,
                   Vector* zVector, Vector* z2Vector, Vector* dVector,
                   int elementsCount, int count, int degree, double lambdaMin, double lambdaMax,
                   double allowableResidual, int minIteration, int maxIteration, int rule,
                   int* iteration, double* residual, double* residualTrace, int traceCapacity);
/* The same on a row partition, shaped after SolveJacobiParallel.  pVector, zVector and z2Vector are full length (count entries): rows
 * gather them, and the halo of z is exchanged in line before every step (the overlap schedule is not used by this loop); dVector and the
 * other vectors hold the local rows.  p.Ap travels in one all-reduce, r.r and r.z in ONE all-reduce of two doubles behind the
 * polynomial: the stop decision of an iteration is taken behind its polynomial, which costs one wasted application at the very end,
 * and x is the judged iterate.  A rank without rows takes part in every collective.  Every rank must pass the same degree and bounds,
 * and a dinvVector or none: that is not checked.  Every other unusable argument on one rank makes every rank return MGCG_ERROR. */
int SolveChebyshevParallel(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                           Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                           Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* dinvVector /* may be NULL */,
                           Vector* zVector, Vector* z2Vector, Vector* dVector,
                           int count, int countForDevice, int offsetForDevice, int elementsCountForDevice, int minJ, int maxJ,
                           int degree, double lambdaMin, double lambdaMax,
                           double allowableResidual, int minIteration, int maxIteration, int rule,
                           int* iteration, double* residual, double* residualTrace, int traceCapacity);

/* ---- Multi-shift CG: (A + shifts[j] I) x_j = b for k = 1 .. 8 shifts >= 0 from ONE CG recurrence on A (one rank, no preconditioner) ---- */
/* Krylov spaces are shift-invariant: the residual of every shifted system is collinear with the base residual, r_j = zeta_j r, so an
 * iteration is SolveEx's product and r update plus ONE fused vector pass for all columns -- three launches, one matrix pass, whatever k
 * is -- where a caller would otherwise build k shifted matrices and run k solves.  The base iterate is not stored: list the shift 0 for it.
 *   xVector         k * count entries, column j at [j * count, (j + 1) * count); OVERWRITTEN: every x_j starts from 0
 *   bVector         count entries; ApVector, pVector, rVector: count entries of work space each
 *   shiftedPVector  k * count entries of work space (the directions p_j; its layout is internal)
 *   shifts          HOST array of k entries, finite and >= 0; they may repeat and need not be sorted
 *   iteration / residual / status   k entries each, any of them may be NULL; residualTrace: column j at [j * traceCapacity, ...), may be NULL
 * Base recurrence (SolveEx's): alpha_k = r.r / p.Ap ; r = r + (-alpha_k) Ap ; beta_k = r.r_new / r.r ; p = r + beta_k p.  Per column,
 * with zeta_{-1} = zeta_0 = 1, alpha_{-1} = 1, beta_{-1} = 0 and p_j = b at the start:
 *   zeta_new = zeta_k zeta_{k-1} alpha_{k-1} / ( alpha_{k-1} zeta_{k-1} (1 + sigma_j alpha_k) + alpha_k beta_{k-1} (zeta_{k-1} - zeta_k) )
 *   alpha_j  = alpha_k (zeta_new / zeta_k) ;  beta_j = beta_k (zeta_new / zeta_k)^2
 *   x_j = x_j + alpha_j p_j (the old p_j) ;  p_j = zeta_new r_new + beta_j p_j
 * Rounding contract: every product is rounded into a double of its own before the add that follows it and nothing is fused into an FMA;
 * the scalar expressions are evaluated in exactly this order --
 *   num = (zeta_k * zeta_{k-1}) * alpha_{k-1}
 *   den = (alpha_{k-1} * zeta_{k-1}) * (1 + sigma_j * alpha_k)  +  (alpha_k * beta_{k-1}) * (zeta_{k-1} - zeta_k)
 *   zeta_new = num / den ; ratio = zeta_new / zeta_k ; alpha_j = alpha_k * ratio ; beta_j = beta_k * (ratio * ratio)
 * -- and x_j = x_j + (alpha_j * p_j), p_j = (zeta_new * r) + (beta_j * p_j).  For sigma_j = 0 this gives zeta = 1.0, alpha_j = alpha_k and
 * beta_j = beta_k exactly: a shift-0 column is SolveEx's x (from x = 0) bit for bit, and so are its trace, iteration and residual under
 * dot_order = 1, where the loop's two dots are the serial sums; the per-column residuals need no sums of their own.
 * Stop rules: the five of SolveEx per column, on the column's residual zeta_new r_new: they see (zeta_new * zeta_new) * (r.r) where SolveEx
 * sees r.r, |zeta_new| * max|r| under MGCG_RULE_HANDMADECL, and the common r0.r0 = b.b under MGCG_RULE_VIENNACL.  A column that stops gets
 * its last x update in that iteration and is frozen: nothing touches its x or p_j again, its trace gets no further entry, and the pass
 * no longer streams it.  The loop runs until no column is live.
 * Returns the worst column status (MGCG_NONFINITE > MGCG_MAXIT_EXCEEDED > MGCG_OK).  A breakdown -- p.Ap <= 0 or not finite (the matrix
 * is not positive definite, or b = 0), a zeta_new, alpha_j or beta_j that is not finite (a zeta that
 * underflowed to 0 shows as such one iteration later) -- ends the affected columns with MGCG_NONFINITE in that iteration, before its x
 * update; their x keeps the last good iterate.  MGCG_ERROR with a message, and nothing enqueued, for k outside 1 .. 8, shifts == NULL, a shift that is negative or
 * not finite, a null handle or a vector that is too small.
 * The product is SolveEx's: compression modes and the automatic column tiles apply.  Out of scope: several ranks, preconditioners (they
 * break the shift invariance), a non-zero initial guess, the deferred x update (x_defer) and the placement draw. */
int SolveShifted(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                 Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                 Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* shiftedPVector,
                 int elementsCount, int count, int k, const double shifts[],
                 double allowableResidual, int minIteration, int maxIteration, int rule,
                 int iteration[], double residual[], int status[], double residualTrace[], int traceCapacity);

/* ---- Shared-subspace block CG: k = 1 .. 8 right-hand sides in ONE block Krylov space (one rank, no preconditioner, plain CSR) ---- */
/* O'Leary's block CG in Dubrulle's breakdown-free form (BCGrQ).  SolveBlockEx runs k independent recurrences that share the matrix pass;
 * here every column minimises over the union of the k Krylov spaces, so all columns converge in fewer iterations, for two more block
 * reads/writes per iteration.  Arguments as SolveBlockEx: column j of x and b at [j*count, (j+1)*count), k*count entries each; Ap, p, r:
 * k*count entries of work space whose layout is internal (row-interleaved T = A S, the search block S, the orthonormal residual block Q).
 * The initial guess in x is honoured (MGCG_RULE_SIMPLE starts from 0, as everywhere).  *iteration: the one common counter (may be NULL);
 * residual[] / status[]: k entries each, may be NULL; residualTrace (may be NULL): column j's trace at j*traceCapacity.
 * Method, with k x k matrices C, alpha, M, zeta (row-major) --
 *   start:  R = B - A X ;  R^T R = U^T U (Cholesky, U upper triangular) ;  Q = R U^-1 ;  C = U ;  S = Q ;  rr0_j = sum_i C[i][j]^2
 *   1. T = A S ;  G = S^T T                               2. G = Ug^T Ug ;  alpha = G^-1 ;  M = alpha C
 *   3. X = X + S M ;  W = Q - T alpha ;  H = W^T W        4. H = zeta^T zeta ;  C = zeta C ;  rr_j = sum_i C[i][j]^2 ;  the stop decision
 *   5. Q = W zeta^-1 ;  S = Q + S zeta^T
 * Q stays orthonormal and the columns' sizes travel in C: || r_j || = || C[:, j] ||, no sums of their own.
 * Rounding contract: every product is rounded into a double of its own before the add or subtraction that follows it, nothing is fused into
 * an FMA, sqrt and / are the correctly rounded ones.  A row of A adds its products in stored order from +0.0 (CsrMVBlock).  Every sum over k
 * terms -- a row of a block times a k x k matrix, a k x k product, rr_j -- starts with its FIRST product and adds the others left to
 * right, l = 0 .. k-1, structural zeros included:  (S M)[i][j] = ((S[i][0] M[0][j] + S[i][1] M[1][j]) + ...), X[i][j] = X[i][j] + (S M)[i][j],
 * W[i][j] = Q[i][j] - (T alpha)[i][j], S[i][j] = Q[i][j] + sum_l S[i][l] zeta[j][l].  Only the upper triangle (a <= b) of a Gram matrix is
 * summed, entry (a, b) = sum over the rows i of left[i][a] * right[i][b].  Cholesky, row i = 0 .. k-1:  d = G[i][i] - U[0][i]^2 - ... -
 * U[i-1][i]^2 (left to right), U[i][i] = sqrt(d), U[i][j] = (G[i][j] - U[0][i] U[0][j] - ... - U[i-1][i] U[i-1][j]) / U[i][i] for j > i.
 * Inverse V of an upper triangular U, column j:  V[j][j] = 1 / U[j][j] ;  for i = j-1 .. 0:  V[i][j] = -(U[i][i+1] V[i+1][j] + ... +
 * U[i][j] V[j][j]) / U[i][i].  alpha[a][b] = alpha[b][a] = V[a][b] V[b][b] + V[a][b+1] V[b][b+1] + ... + V[a][k-1] V[b][k-1] (a <= b, V = Ug^-1).
 * In the default mode a Gram entry is a tree sum of per-workgroup partial sums in a fixed order (the same bits on every run); under
 * dot_order = 1 it is one serial left-to-right sum over the rows, and the whole loop is then a fixed sequence of IEEE operations.
 * Stopping: the four 2-norm rules of SolveEx, evaluated per column in step 4 on (rr_j, rr0_j) with the common counter.  The loop ends in
 * the first iteration in which NO column's decision is "continue"; until then every column is updated (the search space is shared: nothing
 * is frozen), and status[j] / residual[j] are those of that last iteration.  MGCG_RULE_HANDMADECL is refused: it needs max|r|, and R is
 * never formed.
 * Breakdown: a Cholesky pivot that is not finite and > 0 -- in R0^T R0 (dependent or zero initial residual columns: two equal right-hand
 * sides, b_j = 0, an x_j that already solves its system), in S^T A S (the matrix is not positive definite) or in W^T W -- ends the call with
 * MGCG_NONFINITE for every column.  The raw pivot is tested, no tolerance; there is no rank-revealing deflation.  x keeps the last completed
 * iterate: the caller's x, bit for bit, for the first factorisation; the previous iteration's for S^T A S; for W^T W the x of step 3 of that
 * iteration (a valid iterate whose residual norm is unknown).  MgcgGetLastError names the factorisation and the pivot index.  A caller whose
 * right-hand sides may be dependent falls back to SolveBlockEx, whose columns are independent.
 * Returns the worst column status (MGCG_NONFINITE > MGCG_MAXIT_EXCEEDED > MGCG_OK); MGCG_ERROR with a message, and nothing enqueued, for k
 * outside 1 .. 8, a null handle, a vector that is too small, or the max-norm rule.  The matrix is always read as plain CSR, whatever the
 * handle's compression mode; placement draw and x_defer do not apply. */
int SolveBlockKrylov(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
                     Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                     Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector,
                     int elementsCount, int count, int k,
                     double allowableResidual, int minIteration, int maxIteration, int rule,
                     int* iteration, double residual[], int status[], double residualTrace[], int traceCapacity);

/* ---- Mixed-precision CG: an fp32 recurrence corrected by fp64 reliable updates (one rank, no preconditioner, plain CSR) ---- */
/* The CG loop is bound by memory traffic, and an fp32 iteration moves 100 bytes per row of a 7-point matrix where the fp64 one moves 168.
 * SolveMixed runs the recurrence in fp32 and, every few iterations, recomputes the true residual b - A x in fp64 from the fp64 matrix and
 * folds the fp32 partial solution into the fp64 iterate (Sleijpen / van der Vorst reliable updates).  The search direction is kept across
 * an update: the Krylov recurrence is not restarted.  The caller gets an fp64-accurate x and a stop test on a true fp64 residual.
 *
 * MgcgMixedSetup writes (float)a for each of the elementsCount stored values into elements32Vector: a caller-owned double Vector of at
 * least (elementsCount + 1) / 2 entries, read as floats by SolveMixed (as dinvVector is MgcgJacobiSetup's).  *exact (may be NULL) is 1
 * when every value converted without rounding, as the Poisson stencils' do.  A value that is not finite as a float (beyond 3.4e38, an
 * infinity or a NaN) makes the call fail: it returns -1, MgcgGetLastError names the first row that holds one, and the vector must not be
 * handed to a solve.  The check runs on the device and is read back once.  Returns 0 on success. */
int MgcgMixedSetup(MgcgSparse* cusparse, Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                   int elementsCount, int count, Vector* elements32Vector, int* exact);
/* y = A32 x in fp32 on raw device pointers (what CsrMVBlock is to the block product): the product of SolveMixed's iteration, without its
 * p.Ap epilogue.  Every product is rounded to float, never fused with the add.  Up to a mean row length of 20 a row is summed in stored order
 * from +0.0f (bit-exact in every mode); longer rows are summed by 8, 16 or 32 lanes (lane l adds entries l, l + L, ... and the lanes'
 * sums meet in a tree), or in stored order under dot_order = 1. */
void CsrMVFloat(MgcgSparse* cusparse, MgcgMatDescr* matDescr, float* y, const float* elements32, const int* rowOffsets,
                const int* columnIndeces, const float* x, int elementsCount, int count);
/* SolveEx's arguments plus elements32Vector (what MgcgMixedSetup wrote) and *reliableUpdates (may be NULL: the number of updates done).
 * xVector: fp64, the initial guess and the result (MGCG_RULE_SIMPLE starts from 0).  rVector receives the last true fp64 residual.
 * ApVector and pVector are accepted for the class surface's sake and not touched.  The fp32 work vectors xs, r32, p32, Ap32 are the
 * library's, on the handle's workspace, allocated before anything is enqueued.
 * Operation order -- every product is rounded in its own format before the add that follows it, nothing is fused into an FMA:
 *   start       r = b - A x in fp64 (SolveEx's residual product) ; rr0 = rr = maxrr = r.r ; r32 = (float)r ; p32 = r32 ; xs = 0 ; want = 0
 *   iteration it
 *     Ap32 = A32 p32        products rounded to float, a row summed in float (CsrMVFloat)
 *     pAp = sum_i (double)p32_i * (double)Ap32_i                the terms are exact in fp64
 *     alpha = rr / pAp in fp64 ; alpha32 = (float)alpha
 *     xs = xs + (alpha32 * p32) ; r32 = r32 + ((-alpha32) * Ap32)                    in float
 *     rn = sum_i (double)r32_i * (double)r32_i ; maxrr = max(maxrr, rn)
 *     want rises when rn < 0.01 * maxrr, or when the stop rule (below) would end the loop on rn: converged, or the iteration limit
 *   update slot -- only in iterations with it % 4 == 3, and only when want is up:
 *     x = x + (double)xs ; xs = 0 ; r = b - A x with the fp64 matrix ; rn = r.r in fp64 ; r32 = (float)r ; maxrr = rn ;
 *     *reliableUpdates + 1 ; want = 0 ; THE STOP RULE IS DECIDED HERE AND ONLY HERE, SolveEx's rule on the true rn
 *   end         beta = rn / rr in fp64 ; beta32 = (float)beta ; p32 = r32 + (beta32 * p32) ; rr = rn
 * The period 4 and the drop 0.01 (delta = 0.1) are compiled in; no knob changes a result.  In the default mode a sum is a tree sum of
 * per-workgroup partial sums in a fixed order (the same bits on every run); under dot_order = 1 pAp, rn and the update's r.r are serial
 * left-to-right sums and the whole loop is a fixed sequence of IEEE operations (tests/test_mixed_host.py has it in numpy).
 * Stop rules: the four 2-norm rules of SolveEx, on (rn, rr0) of an update with that iteration's counter.  *iteration, *residual, the
 * returned status and the trace entry of an iteration with an update are therefore always those of a true fp64 residual; an iteration
 * without one records the recurrence's sqrt(rn) in the trace (sqrt(rn / rr0) under MGCG_RULE_VIENNACL).  Since only every fourth
 * iteration can stop the loop, *iteration may lie up to 3 beyond the first iteration at which SolveEx's test would have passed, and
 * MGCG_MAXIT_EXCEEDED is reported at the first slot behind maxIteration.
 * MGCG_NONFINITE: p.Ap <= 0 or not finite (the matrix is not positive definite, or the residual is 0), or an alpha32 that is not finite
 * (a p.Ap so small that alpha leaves the fp32 range), ends the loop in that iteration,
 * before its updates -- x keeps its last folded iterate, r the last true residual, and *residual is the recurrence's; a true residual
 * that is not finite, or whose 2-norm is not below 3.4028e38, the range in which every (float)r_i is finite, ends it in its update (the
 * residual is not scaled before conversion).
 * MGCG_ERROR with a message, and nothing enqueued, for MGCG_RULE_HANDMADECL (the recurrence carries no max|r|), an unknown rule, a null
 * handle or a vector that is too small, elements32Vector included.  Out of scope: several ranks, preconditioners, the compressed matrix
 * forms (the matrix is read as plain CSR in both precisions, whatever the handle's compression mode), x_defer and the placement draw. */
int SolveMixed(MgcgBlas* cublas, MgcgSparse* cusparse, MgcgMatDescr* matDescr,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector, Vector* ApVector, Vector* pVector, Vector* rVector, Vector* elements32Vector,
               int elementsCount, int count,
               double allowableResidual, int minIteration, int maxIteration, int rule,
               int* iteration, double* residual, int* reliableUpdates, double* residualTrace, int traceCapacity);

/* Fixed number of CG iterations with no stop test and no host synchronisation inside (bench.py's
 * "steps"): runs `steps` more iterations of the recurrence held in x,r,p (call with restart != 0 first
 * to compute r = b - A x, p = r, rr).  comm may be NULL.  Returns the residual after the last step. */
double CgSteps(MgcgComm* comm, MgcgBlas* cublas, MgcgSparse* cusparse,
               Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
               Vector* xVector, Vector* bVector,
               Vector* ApVector, Vector* pVector, Vector* rVector,
               int count, int countForDevice, int offsetForDevice, int elementsCountForDevice,
               int minJ, int maxJ, int steps, int restart);

/* Extreme eigenvalues by `steps` Lanczos steps on the device (SpMV + dot kernels of the CG path): of A, or with
 * jacobiScaled != 0 of D^-1/2 A D^-1/2 (the spectrum of D^-1 A, what the Jacobi smoother's damping depends on).
 * Scalable counterpart of the reference's dense Jacobi-rotation GetEigenValues
 * (Mgcg/HandmadeCL/MgcgCL/SparseMatrix.cs:234-372).  Ritz values lie inside the spectrum: lambdaMax is approached
 * from below, lambdaMin from above.  ritz (optional) receives the *stepsDone Ritz values in ascending order (room for
 * `steps`).  The start vector is a fixed function of `seed`.  Returns MGCG_OK or MGCG_ERROR. */
int MgcgEstimateSpectrum(MgcgBlas* cublas, MgcgSparse* cusparse,
                         Vector* elementsVector, VectorInt* rowOffsetsVector, VectorInt* columnIndecesVector,
                         int elementsCount, int count, int jacobiScaled, int steps, unsigned seed,
                         double* lambdaMin, double* lambdaMax, double ritz[], int* stepsDone);

/* How the last multi-rank solve on the calling thread scheduled its halo: returns 1 and the local row range
 * [interior[0], interior[1]) that was multiplied while the halo of p travelled on the communicator's own stream
 * (rows outside it wait for the halo), or 0 when the exchange ran in line (single rank, MGCG_OVERLAP=0, or the
 * slice has too few rows that reference local columns only).  interior may be NULL. */
int MgcgLastOverlap(long long interior[2]);
/* The calling thread's last placement draw (tuning knob `placement`): which = 0 the SpMV's output vector Ap, 1 its gathered input p.
 * Returns the number of candidate allocations timed (0: no draw happened -- small vector, knob off, address already exported),
 * milliseconds[i] = the loop's SpMV on candidate i (candidate 0 is the allocation the vector came with), *chosen = the one kept.
 * milliseconds / chosen may be NULL. */
int MgcgLastPlacement(int which, double milliseconds[], int capacity, int* chosen);
/* The measurement behind that choice (overlap = 1): returns 1 and microseconds[0] = one halo exchange in line, microseconds[1] = one
 * fork / empty launch / join round trip, both averaged over the ranks, if the calling thread's last plan was decided by measurement;
 * 0 if it was decided by the knob or the slice's size alone.  microseconds may be NULL. */
int MgcgLastOverlapTimes(double microseconds[2]);
/* Which folds the calling thread's LAST V-cycle took (Apply / SolveMg / SolveMgParallel): bit 0 = on some level the first sweep from
 * zero was formed per gather of the residual pass instead of being stored, bit 1 = on some level the prolongation was formed per gather
 * of the post-smoothing sweep as well (V(1,1), plain CSR, uniform diagonal, power-of-two nx and ny), bit 2 (4) = several ranks: the
 * deep-halo cycle ran (one exchange per coarse level instead of one per pass; knob deep_halo), bit 3 (8) = ... and the finest level's
 * right-hand side carried its halo planes, so every level ran the single-rank folded kernels (SolveMgParallel keeps r in the hierarchy's
 * buffer; MgApply on a caller's vector cannot; taken only when ALL ranks agreed at set-up that their rows hold one and the same uniform
 * diagonal -- the form decides what the level exchanges, r or the stored first sweep).  Schedules only: the results are bit-identical either way (MGCG_NO_FOLD=1 /
 * MGCG_FOLD_UP=0 switch the folds off; MGCG_FOLD_UP=1 takes the second one on levels of any size, by default it is taken up to 100 M rows). */
int MgcgLastVcycleFolds(void);
/* The calling thread's last halo exchange: returns 1 if it moved per-peer index lists (unstructured slices: only the entries
 * of p the slice's column ids reference -- plan built once from them), 0 if contiguous ranges (banded / stencil slices,
 * the reference's [minJ, offset) and [offset + count, maxJ]: Mgcg.cu:83-84, ConjugateGradientParallelGpu.cs:397-398);
 * volume[0] = entries this rank received per exchange, volume[1] = entries the contiguous ranges would have received. */
int MgcgLastHalo(long long volume[2]);
/* Test hook (no device needed): the order in which the lane = row SpMV kernels walk their tiles of `tileRows` rows with
 * `workgroups` workgroups when the far band of the matrix lies `periodRows` rows from the diagonal (0: unknown).
 * tiles[wg * maxTrips + t] = tile of workgroup wg in trip t, or -1; returns 0 (memory order), 1 / 2 (z sweep), -1 (bad arguments). */
int MgcgDebugTileOrder(long long rows, int periodRows, int workgroups, int tileRows, int* tiles, int maxTrips);

#ifdef __cplusplus
}
#endif
#endif /* MGCG_GPU_H */
