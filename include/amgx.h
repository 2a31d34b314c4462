/* amgx.h -- C ABI of the MI355X-native AMG apply path (libngsamg_hip.so).
 *
 * Drop-in boundary for the hot path of LukasKogler/NgsAMG: one preconditioner application
 *     BaseAMGPC::Mult(b, x)            reference src/base/precond/amg_pc.cpp:467-470
 *       -> AMGMatrix::Mult -> SmoothV  reference src/base/solve/amg_matrix.cpp:377-378, 160-307
 * and the pieces reachable through the reference's Python surface (GetSmoother(level).Smooth,
 * GetAMGMatrix().GetMatrix(level), DOFMap transfers).  An NGSolve-side subclass of ngcomp::Preconditioner
 * (or the stand-alone Python module ngsamg_amd.NgsAMG) forwards to these entry points; INTEGRATION.md shows
 * the binding.  Plain pointers and sizes only -- no torch / HIP types in the signatures (streams travel
 * as void*).
 *
 * Lifetime: amgx_create copies every host array of the descriptor to the GPU once (the descriptor is
 * borrowed during the call only).  A handle is not re-entrant (like AMGMatrix::Mult, which mutates its
 * work vectors) but distinct handles are independent.
 *
 * Errors: every function returns 0 on success, non-zero otherwise; amgx_last_error(handle) (handle may
 * be NULL for create-time errors) returns the message.  The shim rethrows it (reference: ngcore::Exception).
 *
 * All vectors are fp64, AoS block vectors (entry = bs*dof + comp; reference amg_matrix.cpp:494).
 */
#ifndef NGSAMG_AMGX_H
#define NGSAMG_AMGX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* host (block-)CSR view: layout of NGSolve SparseMatrix<Mat<br,bc>> */
typedef struct amgx_matrix {
  int64_t n_rows, n_cols;     /* block rows / block columns                           */
  int32_t br, bc;             /* block height / width (1, 2, 3, 6; P: 3x6, PT: 6x3)    */
  const int64_t* rowptr;      /* [n_rows+1] (size_t firsti in the reference)          */
  const int32_t* col;         /* [nnz] ascending per row                              */
  const double* val;          /* [nnz*br*bc] row-major blocks                         */
} amgx_matrix;

/* smoother kinds = ngs_amg_sm_type (reference src/base/precond/amg_pc.cpp:1033-1138) */
enum {
  AMGX_SM_JACOBI = 0,         /* JacobiSmoother<TM>, base_smoother.cpp:61-114         */
  AMGX_SM_GS = 1,             /* Gauss-Seidel (GSS3, gssmoother.cpp:196-398) executed as multicolour GS */
  AMGX_SM_BGS = 2,            /* block Gauss-Seidel over aggregate blocks (BSmoother, block_gssmoother.cpp:17-498), */
                              /*   blocks of one colour relaxed in parallel (the reference's sm_shm sweep does too) */
  AMGX_SM_CHEBY = 3           /* Chebyshev polynomial smoother in the (block-)Jacobi-preconditioned operator Dinv A (no reference */
                              /*   counterpart; an own option).  Degree k on [lmin, lmax], lmin = lmax / ratio:                    */
                              /*     theta = (lmax+lmin)/2, delta = (lmax-lmin)/2, sigma = theta/delta, rho_1 = 1/sigma            */
                              /*     step 1:        d = (1/theta) Dinv r,  x += d                                                  */
                              /*     step j = 2..k: rho_j = 1/(2 sigma - rho_{j-1}),  d = rho_j rho_{j-1} d + (2 rho_j/delta) Dinv (b - A x),  x += d */
                              /*   r of step 1 follows the flag contract of amgx_smooth (b from zero, res when updated, else b - A x); */
                              /*   Smooth == SmoothBack; sm_steps / sm_symm compose as for every smoother.  Not on rank-partitioned levels. */
};
enum { AMGX_CYCLE_V = 0, AMGX_CYCLE_W = 1, AMGX_CYCLE_BS = 2 };   /* ngs_amg_mg_cycle, amg_matrix.hpp:37-43 */
enum { AMGX_CLEV_NONE = 0, AMGX_CLEV_INV = 1 };                   /* ngs_amg_clev,     amg_matrix.cpp:217-247 */

/* flags for the vector arguments of the calls below */
enum {
  AMGX_HOST_PTR = 0,          /* vectors are host arrays: copied H2D / D2H inside the call            */
  AMGX_DEVICE_PTR = 1,        /* vectors are device arrays on the handle's GPU (no copies)            */
  AMGX_NO_GRAPH = 2,          /* launch the kernels directly instead of replaying the captured graph  */
  AMGX_PCG_SINGLE_REDUCTION = 16, /* amgx_pcg / amgx_dist_pcg with a preconditioner: the Chronopoulos / Gear form of the   */
                              /* same recurrence -- ONE reduction point (one all-reduce of two scalars) per iteration and  */
                              /* three launches beside the cycle and the level-0 product instead of five; histories agree   */
                              /* with the classical form to ~1e-6                                                            */
  AMGX_MULTI_INTERLEAVED = 32,/* multi-vector calls: entry (row i, column j) of a multi-vector lives at i*k + j and ld is      */
                              /* ignored.  Without it: column-major, column j starts at j*ld, ld >= level size                */
  AMGX_MULTI_FUSE = 64,       /* amgx_apply_multi / amgx_matvec_multi / amgx_pcg_multi: run fused column groups on every handle */
                              /* that qualifies under the EXTENDED rule (Chebyshev and block levels, see below); a handle that  */
                              /* does not qualify runs the column loop -- never an error.  Without it every call is as before   */
  AMGX_MULTI_FUSE_GS = 128,   /* the same calls, amgx_smooth_multi, amgx_multi_plan / amgx_multi_note: implies AMGX_MULTI_FUSE   */
                              /* and admits scalar Gauss-Seidel levels (block-hybrid or multicolour form, see below) as well; a  */
                              /* handle that does not qualify runs the column loop.  Without it every call is as before, calls   */
                              /* that carry AMGX_MULTI_FUSE alone included                                                       */
  AMGX_MULTI_FUSE_GS_BLOCK = 256,/* accepted wherever AMGX_MULTI_FUSE_GS is; implies it and AMGX_MULTI_FUSE, and admits          */
                              /* Gauss-Seidel on 2x2 / 3x3 / 6x6 levels (hybrid-block, block-coloured, multicolour forms, see     */
                              /* below) as well; never an error: a handle that does not qualify runs the column loop.  Without   */
                              /* it every call is as before, calls that carry the two flags above included                      */
  AMGX_MULTI_FUSE_DOWN = 512, /* the multi-vector calls: a fused column group runs the down pass of every level that qualifies  */
                              /* as the single-vector fused down kernel on interleaved vectors (see "multi-vectors" below); it   */
                              /* implies nothing and never causes an error.  Without it every call is as before                  */
  AMGX_MULTI_FUSE_DOWN_DIA = 1024,/* accepted wherever AMGX_MULTI_FUSE_DOWN is; implies it (and nothing else) and admits levels  */
                              /* whose fused down launch reads the symmetric diagonal image, 512-row or box chunks (see below);   */
                              /* never an error.  Without it every call is as before, calls that carry AMGX_MULTI_FUSE_DOWN      */
                              /* included                                                                                        */
  AMGX_MULTI_FUSE_F32 = 2048, /* accepted wherever AMGX_MULTI_FUSE_GS is; implies nothing and is never an error.  With it a      */
                              /* Gauss-Seidel level whose sweeps read single-precision images no longer keeps the handle in the   */
                              /* column loop under AMGX_MULTI_FUSE_GS (scalar levels) / AMGX_MULTI_FUSE_GS_BLOCK (2x2 / 3x3 / 6x6    */
                              /* levels), where the multi-vector kernels exist on the float arrays (see below).  Without it     */
                              /* every call is as before                                                                         */
  AMGX_MULTI_FUSE_DOWN_F32 = 4096 /* accepted wherever AMGX_MULTI_FUSE_DOWN is; implies it and AMGX_MULTI_FUSE_F32 (and nothing  */
                              /* else: the Gauss-Seidel bits stay the caller's) and admits scalar Gauss-Seidel levels with        */
                              /* single-precision images to the fused down pass, the local-window form of `rest` included (see    */
                              /* below); never an error.  Without it every call is as before, calls that carry                    */
                              /* AMGX_MULTI_FUSE_DOWN | AMGX_MULTI_FUSE_F32 included                                               */
};

typedef struct amgx_level_desc {
  amgx_matrix A;              /* level matrix (smoothers[l]->GetAMatrix())                           */
  amgx_matrix P, PT;          /* ProlMap<TM>: P and explicit P^T (dof_map.hpp:252-334); empty on the coarsest */
  const double* dinv;         /* [n*bs*bs] inverted block diagonal, 0 on non-free rows (gssmoother.cpp:143-170) */
  const uint8_t* free_dofs;   /* [n] 1 = free block row, or NULL (all free)                           */
  int32_t sm_type;            /* AMGX_SM_*                                                           */
  double omega;               /* Jacobi damping, reference default 0.9 (base_smoother.hpp:279)       */
  int32_t sm_steps;           /* ngs_amg_sm_steps (ProxySmoother, base_smoother.hpp:169-229)         */
  int32_t sm_symm;            /* ngs_amg_sm_symm                                                     */
  const int32_t* color;       /* [n] colour of each free row (required for AMGX_SM_GS), -1 otherwise  */
  int32_t n_colors;
  /* AMGX_SM_BGS only (amgh_bgs_dinv / amgh_bgs_coloring produce these): */
  int32_t bgs_n_blocks;
  const int32_t* bgs_block_ptr;   /* [n_blocks+1]; block k owns bgs_block_rows[ptr[k] .. ptr[k+1]) (disjoint sets)   */
  const int32_t* bgs_block_rows;
  const int64_t* bgs_dinv_ptr;    /* [n_blocks+1] offsets into bgs_dinv                                             */
  const double* bgs_dinv;         /* per block the dense inverse of its diagonal block, M x M column-major, M = bs*size */
  const int32_t* bgs_color;       /* [n_blocks] colour of each block; coupled blocks must differ                    */
  int32_t bgs_n_colors;
  amgx_matrix Q;              /* optional (rowptr == NULL: none).  Folded post-smoothing prolongation                */
                              /*   Q = (I - omega*Dinv*A) P  of a Jacobi level of the V-cycle, n_rows x (coarse n_cols). */
                              /*   Square levels: the library builds it itself.  Rank-partitioned levels (A has ghost  */
                              /*   columns): the caller, who holds the P rows of the ghost vertices, supplies it; its    */
                              /*   columns index the coarse level's [owned | ghost] vector (see amgx_cycle_up).          */
  int32_t gs_block_rows;      /* AMGX_SM_GS, scalar levels: 0 = multicolour Gauss-Seidel over the whole level (one launch per  */
                              /*   colour); B > 0 = BLOCK-HYBRID Gauss-Seidel, one launch per sweep: blocks of B consecutive  */
                              /*   rows (B = 1024, 512, ..., 64) are swept like the ranks of the reference's hybrid smoother   */
                              /*   (gssmoother.cpp:709-861): GS inside a block in colour order, couplings that leave the block */
                              /*   frozen at their sweep-start values.  `color` then only has to separate coupled rows of the  */
                              /*   SAME block (amgh_coloring_blocked) and `dinv` should be the inverse of the l1-modified      */
                              /*   diagonal (amgh_hybrid_dinv).  Rows may have at most 16 * (1024 / B) + 1 entries.            */
                              /*   Square-block levels (2x2, 3x3, 6x6): B = block rows per workgroup (amgh_hybrid_dinv_block).  */
  const int32_t* gs_block_ids;/* optional, square-block levels with gs_block_rows = B > 0: [n] sweep block of every block row   */
                              /*   (ids 0 .. n_blocks-1, at most B rows per block) instead of runs of B consecutive rows --     */
                              /*   compact blocks (amgh_compact_blocks) freeze fewer couplings, like the mesh-partitioner        */
                              /*   subdomains of the reference's hybrid smoother; colours from amgh_coloring_blockids, dinv     */
                              /*   from amgh_hybrid_dinv_block_ids                                                              */
  const int32_t* gs_block_color;/* optional, square-block levels with gs_block_rows = B > 0: [n] colour of the SWEEP BLOCK of every  */
                              /*   block row (a colouring of the block graph, amgh_bgs_coloring: coupled blocks differ; constant     */
                              /*   inside a block).  A sweep is then one launch per block colour, in place: exact Gauss-Seidel in    */
                              /*   the order (block colour, block, in-block colour) -- GSS3's loop (gssmoother.cpp:196-257) in a      */
                              /*   parallel order -- instead of the hybrid form's frozen couplings between blocks; `dinv` is then     */
                              /*   the plain (pseudo-)inverse of the diagonal blocks (amgh_calc_dinv), no l1 modification.            */
  int32_t gs_n_block_colors;  /*   number of block colours (0: none, hybrid form)                                                    */
  /* AMGX_SM_CHEBY only; zero-initialised = defaults: */
  int32_t cheb_degree;        /*   1 .. 8 steps per smooth (0: 2)                                                                    */
  double cheb_lambda_max;     /*   upper end of the interval (0: 1.1 x a 30-step power-iteration estimate of lambda_max(Dinv A),     */
                              /*   computed by amgx_create on the device; amgx_smoother_info reports it)                             */
  double cheb_ratio;          /*   lmin = lmax / ratio, ratio > 1 (0: 10)                                                            */
  int32_t mat_prec;           /* AMGX_PREC_*: storage of the values of A that the smoother passes of this level read (0 = fp64, today's  */
                              /*   behaviour).  AMGX_PREC_F32, levels smoothed with AMGX_SM_CHEBY only (an error on any other smoothed    */
                              /*   level; ignored on the coarsest of several): amgx_create keeps a second image of A whose values are float, the     */
                              /*   fp64 image rounded to nearest with every index array shared (+ half of A's value bytes of device      */
                              /*   memory).  Every product with A that the SMOOTHER and the CYCLE launch reads it: the Chebyshev steps,    */
                              /*   the residual before the restriction (fused form included) and update_res of amgx_smooth.  All vectors, */
                              /*   dinv, the transfers and the accumulation stay fp64: the result is the fp64 cycle on the rounded A.      */
                              /*   amgx_matvec, amgx_residual, amgx_matvec_multi, the level-0 operator of amgx_pcg / amgx_gmres /          */
                              /*   amgx_pcg_multi and the lambda_max estimate keep the fp64 image: a solve converges to the solution of    */
                              /*   the TRUE system and amgx_smoother_info is that of the double handle.  Images: A in plain sliced-ELL or  */
                              /*   block sliced-ELL form; levels in another format (CSR-vector, windowed, block CSR: the small ones) stay  */
                              /*   fp64 silently -- amgx_matrix_info(which = 7) tells.  A value that rounds to +-inf is an error.          */
                              /*   Environment of amgx_create: AMGX_NO_MAT_F32=1 ignores every request.                                    */
                              /*   AMGX_PREC_F32 is also accepted on square-block levels smoothed with AMGX_SM_GS (an error on Jacobi,     */
                              /*   AMGX_SM_BGS and scalar Gauss-Seidel levels and on rank-partitioned levels).  On a 2x2, 3x3 or 6x6       */
                              /*   level whose sweeps run in the hybrid-block, block-coloured or multicolour BSELL form, every BSELL       */
                              /*   image that the sweeps and the residual after the sweep from zero read -- A itself included -- gets a    */
                              /*   float twin (each image's fp64 value rounded to nearest, index arrays shared); dinv stays that of the    */
                              /*   true A.  update_res -- the residual of an iterate that a further correction uses: W / BS cycles,        */
                              /*   amgx_smooth -- reads the fp64 A, where the rounded one would shift the result by cond(A) * 6e-8. The    */
                              /*   result is that of the fp64 kernels on the rounded images, bit for bit.  Gauss-Seidel levels in any      */
                              /*   other form (the row list over block CSR, other block sizes) stay fp64 silently -- amgx_level_extra      */
                              /*   entries 9 .. 11 tell.  AMGX_GS_F32_WIDE=1 at amgx_create: no float images; the rounded values are       */
                              /*   written into fp64 images of exactly those levels and the fp64 kernels run (A/B twin).                   */
                              /*   AMGX_PREC_F32_SCALAR_GS (2): single-precision images for Gauss-Seidel on a SCALAR       */
                              /*   level.  Accepted on a smoothed level with sm_type = AMGX_SM_GS, block size 1 and n_cols == n_rows; an    */
                              /*   error that names the level and mat_prec on any other smoother, on a block level and on a level with     */
                              /*   ghost columns (amgx_dist_create: "rank-partitioned"); ignored on the coarsest level of several, taken   */
                              /*   by the only level of a single-level handle.  After the level's Gauss-Seidel images exist, each of the   */
                              /*   block-hybrid images full, fullLW, lowin, rest, restLW or of the multicolour images sell, lower, upper   */
                              /*   that the level has gets a float value array: the stored fp64 values rounded to nearest, every index     */
                              /*   array, rowid, slotcolor and the window lists shared.  The fp64 value arrays of these images are         */
                              /*   released.  dinv, cvec (1 / dinv - a_kk), all vectors, P, P^T, the chunk-local restriction data, the     */
                              /*   tail program's copies and the dense tail stay fp64 and true: with the split images the diagonal acts    */
                              /*   with its true value, so the handle is not the fp64 cycle on a rounded A; without them (AMGX_GSB_NO_SPLIT;*/
                              /*   multicolour without the split) it is, bit for bit.  A itself gets an image only on a level without     */
                              /*   split images, where the residual after the sweep from zero reads A: a float array where A is plain     */
                              /*   sliced-ELL, else rounded values at fp64 width in a separate array.  Read by: the general sweep, the     */
                              /*   sweep from zero, the residual after it in every form (separate, fused with the chunk-local restriction  */
                              /*   on sliced-ELL, row windows or the local window), the colour launches and the upper residual, and        */
                              /*   update_res inside pre-smoothing from zero.  update_res anywhere else, amgx_matvec, amgx_residual,       */
                              /*   amgx_matvec_multi and the Krylov operator read the fp64 A.  A value that rounds to +-inf is an error    */
                              /*   that names the level ("single precision"); nothing half-built is left.  AMGX_NO_MAT_F32=1 ignores the   */
                              /*   request.  AMGX_GS_F32_WIDE=1 (A/B twin): no float arrays; the rounded values are written at fp64 width  */
                              /*   into exactly those images (A: a separate array) and the fp64 kernels run -- same bits.                  */
                              /*   amgx_gs_prec_info tells what was built.                                                                 */
                              /* (jacobi_prec below fills the four bytes that padded the struct after mat_prec: sizeof is unchanged.   */
                              /*  The Python binding, ngsamg_amd/_lib.py, reaches it by that offset and not through its field list; a   */
                              /*  field appended after it must be added there as well.)                                                 */
  int32_t jacobi_prec;        /* AMGX_JACOBI_PREC_*: storage of the matrix images that the passes of a SCALAR JACOBI level read (0 = fp64, */
                              /*   today's behaviour).  Accepted on smoothed scalar levels (block size 1) with sm_type =   */
                              /*   AMGX_SM_JACOBI and n_cols == n_rows; an error that names level and field on another smoother, a block   */
                              /*   level, a rank-partitioned level or a value outside 0 .. 2; ignored on the coarsest level of several.    */
                              /*   AMGX_JACOBI_PREC_F32: after the level's images exist, each of A (plain sliced-ELL), A' (plain           */
                              /*   sliced-ELL), the local-window image of A', the symmetric diagonal image, Q (plain sliced-ELL) and the   */
                              /*   local-window image of Q gets a float value array, the stored fp64 values rounded to nearest, every      */
                              /*   index array shared.  The images are rounded AS STORED (A' holds a_ij * omega * dinv_j, Q holds           */
                              /*   (I - omega Dinv A) P), so the handle is not the fp64 cycle on a rounded A except on the literal paths.  */
                              /*   Images in another format, P, P^T, the restriction data, dinv, the tail program and the dense tail stay  */
                              /*   fp64.  Every product that the Jacobi step and the cycle launch on the level reads the float images:     */
                              /*   the fused down pass, EP_PRE, EP_JAC, the residual before the restriction, Q on the way up, the stage    */
                              /*   entry points amgx_jacobi_pre / amgx_cycle_down / amgx_cycle_up / amgx_jacobi_post, amgx_time_op ops 1,  */
                              /*   5, 6, 7, 8.  update_res (the residual of a non-zero iterate that a further correction uses),            */
                              /*   amgx_matvec, amgx_residual, amgx_matvec_multi and the Krylov operator keep the fp64 A.  The fp64 value  */
                              /*   arrays of A', its local-window form, the diagonal image, Q and its local-window form are released; A    */
                              /*   keeps both.  A value that rounds to +-inf is an error that names the level.                             */
                              /*   AMGX_JACOBI_PREC_F32_WIDE (A/B twin): no float arrays; the same rounded values are written at fp64      */
                              /*   width into exactly those images (A: into a separate array) and the fp64 kernels run -- same bits.       */
                              /*   AMGX_NO_MAT_F32=1 at amgx_create ignores the request.  amgx_jacobi_prec_info tells what was built.      */
} amgx_level_desc;
enum { AMGX_PREC_F64 = 0, AMGX_PREC_F32 = 1 };                    /* amgx_level_desc.mat_prec */
enum { AMGX_PREC_F32_SCALAR_GS = 2 }; /* amgx_level_desc.mat_prec, scalar AMGX_SM_GS levels only */
enum { AMGX_JACOBI_PREC_F64 = 0, AMGX_JACOBI_PREC_F32 = 1, AMGX_JACOBI_PREC_F32_WIDE = 2 };     /* amgx_level_desc.jacobi_prec */

typedef struct amgx_hierarchy_desc {
  int32_t n_levels;
  const amgx_level_desc* levels;
  int32_t cycle;              /* AMGX_CYCLE_*                                                        */
  int32_t clev;               /* AMGX_CLEV_*                                                         */
  int64_t coarse_n;           /* scalar size of the coarsest level                                   */
  const double* coarse_inv;   /* dense [coarse_n^2] inverse on the free dofs (crs_inv, amg_pc.cpp:843-928); NULL with clev = INV:    */
                              /*   amgx_create inverts the coarsest level matrix on its free dofs itself, on the device (blocked     */
                              /*   Gauss-Jordan, trailing updates as f64 MFMA tiles; SPD required; up to AMGX_COARSE_DENSE_MAX =     */
                              /*   16384 unknowns) -- what the host setup leaves to the device beyond 4096 unknowns                  */
  int32_t device;             /* HIP device ordinal                                                  */
  int32_t use_graph;          /* 1: capture each distinct (b, x) cycle into a hipGraph and replay it */
} amgx_hierarchy_desc;

typedef struct amgx_handle_t* amgx_handle;

const char* amgx_last_error(amgx_handle h);

int amgx_create(const amgx_hierarchy_desc* desc, amgx_handle* out);
int amgx_destroy(amgx_handle h);

/* All work of the handle is enqueued on ONE stream.  A new handle owns a private non-blocking stream; this
 * call switches it to the caller's hipStream_t (NULL = the legacy default stream), so that the caller's own
 * kernels and events on that stream order with the preconditioner without host synchronisation. */
int amgx_set_stream(amgx_handle h, void* hip_stream);
int amgx_synchronize(amgx_handle h);

/* x = C b : BaseAMGPC::Mult / AMGMatrix::Mult (amg_pc.cpp:467-470, amg_matrix.cpp:377-378).
 * b_status: 0 = DISTRIBUTED, 1 = CUMULATED (single GPU: both mean the same). */
int amgx_apply(amgx_handle h, const double* b, double* x, int b_status, int flags);
/* x += s * C b : AMGMatrix::MultAdd (amg_matrix.cpp:385-389) */
int amgx_apply_add(amgx_handle h, double s, const double* b, double* x, int flags);

/* smoothers[level]->Smooth (dir = 0) / SmoothBack (dir = 1) with the reference's flag contract
 * (base_smoother.hpp:68-112); goes through the ProxySmoother when sm_steps > 1 or sm_symm. */
int amgx_smooth(amgx_handle h, int level, int dir, double* x, const double* b, double* res,
                int res_updated, int update_res, int x_zero, int flags);
/* AMGMatrix::SmoothVFromLevel (amg_matrix.cpp:310-374) */
int amgx_smooth_v_from_level(amgx_handle h, int level, double* x, const double* b, double* res,
                             int res_updated, int update_res, int x_zero, int flags);
/* Stage entry points for rank-partitioned levels: a level matrix may have n_cols > n_rows, the
 * trailing columns being ghost entries owned by other ranks.  The caller fills the ghost part of the gathered vector
 * (halo exchange, e.g. torch.distributed over RCCL) and drives the cycle stage by stage:
 *   amgx_jacobi_pre : x = omega*Dinv*b, r = b - A x     b: n_cols entries (ghosts valid), x, r: n_rows
 *                     (RichardsonSmoother::Smooth with res_updated = update_res = x_zero = 1, base_smoother.cpp:61-74)
 *   amgx_prolong    : x_out = x_in + fac * P x_coarse   (ProlMap::AddC2F, dof_map.cpp:697-709, out of place)
 *   amgx_jacobi_post: x_out = x_in + omega*Dinv*(b - A x_in)   x_in: n_cols entries (ghosts valid), x_out != x_in */
int amgx_jacobi_pre(amgx_handle h, int level, const double* b, double* x, double* r, int flags);
/* The same two stages in the form the single-GPU V-cycle runs them (fused pre-smoothing + restriction, post-smoothing
 * folded into the prolongation); only for Jacobi levels that have Q (amgx_matrix_info(which = 4) reports it):
 *   amgx_cycle_down : z = S(S0(b)) stored to x (two Jacobi steps from zero WITHOUT coarse correction), and
 *                     b_coarse = P^T (b - A omega*Dinv*b)         b: n_cols entries (ghosts valid); x: n_rows;
 *                     b_coarse: owned rows of the coarse level     (amg_matrix.cpp:193-212)
 *   amgx_cycle_up   : x += Q x_coarse  => x = result of  x_pre + P x_c  followed by the Jacobi post-smoothing step
 *                     x_coarse: Q.n_cols entries (coarse [owned | ghost], ghosts valid)   (amg_matrix.cpp:263-302)
 * One halo exchange per stage (b before down, the coarse x before up) instead of two per level. */
int amgx_cycle_down(amgx_handle h, int level, const double* b, double* x, double* b_coarse, int flags);
int amgx_cycle_up(amgx_handle h, int level, double* x, const double* x_coarse, int flags);
/* r = b - A_level x   (BaseSmoother::CalcResiduum, base_smoother.hpp:132-142); x: n_cols entries, b, r: n_rows.
 * With amgx_smooth (whose x may carry ghost entries too: they are read, never written) this gives the stages of the
 * hybrid Gauss-Seidel smoother of rank-partitioned levels: local sweep on the owned rows with the off-rank values
 * frozen (reference HybridGSSmoother, gssmoother.cpp:709-861, with dinv = inverse of the modified diagonal). */
int amgx_residual(amgx_handle h, int level, const double* x, const double* b, double* r, int flags);
int amgx_jacobi_post(amgx_handle h, int level, const double* x_in, const double* b, double* x_out, int flags);
int amgx_prolong(amgx_handle h, int level, double fac, const double* x_in, const double* x_coarse, double* x_out, int flags);

/* y = A_level x  (GetMatrix(level).Mult); x has n_cols entries */
int amgx_matvec(amgx_handle h, int level, const double* x, double* y, int flags);
/* DOFMap::TransferF2C (x_coarse = P^T x_fine) and AddC2F (x_fine += fac * P x_coarse), dof_map.cpp:636-709 */
int amgx_transfer_f2c(amgx_handle h, int level, const double* x_fine, double* x_coarse, int flags);
int amgx_add_c2f(amgx_handle h, int level, double fac, double* x_fine, const double* x_coarse, int flags);
/* crs_inv->Mult on the coarsest level */
int amgx_coarse_solve(amgx_handle h, const double* rhs, double* x, int flags);

/* GetNLevels / GetNDof / GetBlockSize (python_amg.hpp:15-103) */
int amgx_n_levels(amgx_handle h);
int amgx_level_info(amgx_handle h, int level, int64_t* n, int32_t* bs, int64_t* nnz);
/* how the V-cycle of this handle is launched (no reference counterpart; the reference's cycle is a host loop,
 * amg_matrix.cpp:183-302):  tail_level = first level run inside the single-workgroup tail kernel (-1: none);
 * dense_level = first level of the COLLAPSED coarse levels (-1: none): the sub-cycle on the levels >= dense_level is a
 * fixed linear operator, formed once at amgx_create by running the device's own sub-cycle on the unit vectors and applied
 * as one dense GEMV of dense_n x dense_n doubles (same operator, summation order differs: rounding-level differences).
 * Environment of amgx_create: AMGX_NO_DENSE_TAIL=1 disables, AMGX_DENSE_MAX=<n> caps dense_n (default 8192). */
int amgx_cycle_info(amgx_handle h, int32_t* tail_level, int32_t* dense_level, int64_t* dense_n);
/* the smoother of a level: type (AMGX_SM_*) and, for AMGX_SM_CHEBY, degree, interval and whether amgx_create estimated
 * lambda_max itself (degree = 0, interval = 0 for the other types).  Any output pointer may be NULL. */
int amgx_smoother_info(amgx_handle h, int level, int32_t* sm_type, int32_t* degree, double* lambda_max, double* lambda_min, int32_t* estimated);
/* device-format report per level matrix: which = 0 A, 1 P, 2 PT, 3 A' = A*omega*Dinv (pre-smoothing image),
 * 4 Q = (I - omega*Dinv*A) P (post-smoothing folded into the prolongation), 5 the "local window" image of A' that the fused down
 * kernel of a long-row level reads (chunk-local 16-bit columns, gathered vector staged in LDS), 6 the local-window image of Q
 * (window-local columns, the coarse values of a 512-row window staged in LDS); fmt: -1 not built, 0 CSR-vector,
 * 1 sliced-ELL, 2 block sliced-ELL, 3 sliced-ELL with length-sorted row windows, 5 local-window sliced-ELL, 4 rigid-body transfer blocks (P_ik = w_ik Q(t_ik)
 * stored as (column, w, t): detected block by block at amgx_create, elasticity_energy.hpp:447-490), 6 (which = 3 only) the
 * symmetric diagonal image of A that replaces A' on levels whose A lies on at most 16 diagonals and is symmetric bit for bit
 * (stored_entries = upper diagonals x rows; AMGX_NO_DIA=1 at amgx_create keeps A'); stored_entries counts padding
 * (for the traffic model in DESIGN.md).  which = 7: the single-precision image of A that the smoother passes of a level with
 * mat_prec = AMGX_PREC_F32 read: fmt 1 or 2 (-1: not built), stored_entries and lanes those of A -- 4-byte values, the indices are
 * the ones of which = 0.  `which` outside 0 .. 7 is an error. */
int amgx_matrix_info(amgx_handle h, int level, int which, int32_t* fmt, int64_t* stored_entries, int32_t* lanes_per_row);

/* bytes of matrix data (values, indices, pointers, in the device encoding) that one SpMV with this matrix
 * streams from HBM -- the model value behind "traffic" in DESIGN.md; which as above (7: 4 bytes per stored value + the shared
 * indices and pointers of A; 0 when the level has no single-precision image) */
int amgx_matrix_stream_bytes(amgx_handle h, int level, int which, int64_t* bytes);

/* read-only report of the paths amgx_create chose for one level (changes nothing).  Fills out[0 .. min(n_out, AMGX_LEVEL_PATHS_N)):
 *    0 fused Jacobi down kernel: 0 none, 1 sliced-ELL, 2 sliced-ELL with row windows, 3 local-window sliced-ELL, 4 diagonal image;
 *      5: the fused residual + restriction kernel of a Chebyshev level (sliced-ELL image of A; 1 .. 3 then describe it)
 *    1 its workgroup size (rows per chunk x lanes)      2 its lanes per row (0: none)
 *    3 entries of P per thread of its chunk-local restriction (0: none)
 *    4 chunk form: 0 consecutive rows, 1 compact chunks (chunks of listed slices), 2 box chunks of the diagonal image (a chunk =
 *      a box of whole grid lines, dia_box_pre_restrict_kernel; entry 0 stays 4, entries 1, 5, 6 and 18 describe the boxes)
 *    5 most slots (distinct coarse columns) in one chunk                    6 most entries of P in one chunk
 *    7 upper diagonals K of the diagonal image (0: none)
 *    8 .. 11 remapped workgroup placement (1) of A, A', Q and of the diagonal image
 *   12, 13 slices of A with 16-bit columns, all slices of A (sliced-ELL forms; 0 otherwise)
 *   14, 15 the same for A'
 *   16 chunks of the local-window image of A' that keep global columns (no window)
 *   17 folded post-smoothing (1: the V-cycle runs Q on the way up)
 *   18 chunks of the chunk-local restriction
 *   Gauss-Seidel sweep (0 where the level has none):
 *   19 form: 0 none, 1 multicolour scalar (gs_color_kernel), 2 multicolour block row-list (bgs_color_kernel),
 *      3 multicolour block BSELL (bgs_bsell_color_kernel), 4 block-hybrid scalar (gsb_sweep_kernel),
 *      5 block-hybrid square-block (bgsb_sweep_kernel), 6 block-coloured square-block (bgsb_sweep_kernel per block colour),
 *      7 aggregate block Gauss-Seidel (bgs_block_kernel)
 *   20 lanes per row G (forms 1 and 4)     21 workgroup size of the sweep (forms 1 .. 6)
 *   22 rows per sweep block (form 4: B, forms 5 and 6: block rows BB)
 *   23 colours (in-block colours for forms 4 .. 6)     24 block colours (form 6)
 *   25 split images present (form 1: lower / upper, 3: block lower / upper, 4: lowin / rest, 5 and 6: rest)
 *   26, 27 form 4: widest slice (entries per lane) of the lower in-block image and of the whole image
 *   28 form 4: the sweep from zero takes the narrow kernel (2 entries per lane and pass; otherwise 8)
 *   29 form 4: the general sweep takes the mid-width kernel (5 entries per lane and pass; otherwise 8)
 *   30 form 4: the general sweep reads the local-window image
 *   31 form 2: bitmask of the lanes per block row W (1, 2, 4, 8) its colours launch with
 *   32 form 4: blocks of the local-window image that keep global 32-bit columns
 *   33 form 4: the fused residual + restriction kernel the down pass of the cycle runs after the sweep from zero: 0 none (separate
 *      residual and restriction, also on a level whose down pass is not the plain one-step sweep), 1 sliced-ELL, 2 sliced-ELL with
 *      row windows, 3 local-window sliced-ELL (the image of the couplings the sweep did not use).  (The rank-partitioned driver
 *      calls the same kernels on its own condition; this entry describes the single-rank cycle.)
 *   34, 35, 36 form 7: workgroup size TH and lanes per scalar row G of the bgs_block_kernel<BS, TH, G> the sweep launches, and the
 *      scalar dofs of the largest block they were chosen from
 *   37, 38, 39 the kernel of a product with A, P, P^T held in the block CSR format (0: another format, 1 x 1 blocks or no such
 *      matrix): 100 + W = bcsr_rowlane_kernel with W lane groups per block row, 200 + G = bcsrvec_spmv_kernel with G lanes per
 *      block row
 * Returns 0, or non-zero for a bad level or n_out < 1. */
#define AMGX_LEVEL_PATHS_N 40
int amgx_level_paths(amgx_handle h, int level, int64_t* out, int n_out);

/* further read-only entries of the same kind (amgx_level_paths keeps its 40).  Fills out[0 .. min(n_out, AMGX_LEVEL_EXTRA_N)):
 *    0 operations of the program the single-workgroup tail kernel runs (the same for every level; 0: the cycle has no such tail)
 *    1 form of this level's Gauss-Seidel sweeps inside the tail kernel: 1 x in LDS and the rows in registers, 0 x in global
 *      memory, -1 the level is not part of the tail or its smoother is not Gauss-Seidel
 *    2, 3 multicolour scalar Gauss-Seidel (form 1 of entry 19 above): slices with 16-bit columns and all slices of the
 *      colour-major copies (whole copy + the lower / upper split copies where present; 0 otherwise)
 *    4 ... and whether their 16-bit columns are row-relative (AMGX_GS_ROWREL at amgx_create)
 *    5, 6 sliced-ELL images of A and A': every row stores its diagonal entry first (0 after AMGX_NO_DIAG_FIRST=1, with several lanes
 *      per row, with row windows or in another format)          7 the diagonal slot of A' holds omega instead of A'_ii
 *    8 whole-cycle graphs this handle holds at the moment (the same for every level)
 *    9 the Gauss-Seidel sweeps of this level read single-precision images (1; 0 otherwise, also under AMGX_GS_F32_WIDE)
 *    10, 11 the number of single-precision Gauss-Seidel images of this level (A included) and the bytes of their values
 *      (under AMGX_GS_F32_WIDE: the fp64 images that hold rounded values, 8 bytes per value, while entry 9 stays 0)
 *      (a scalar level with mat_prec = AMGX_PREC_F32_SCALAR_GS reports the same three; amgx_gs_prec_info names the images)
 * Returns 0, or non-zero for a bad level or n_out < 1. */
#define AMGX_LEVEL_EXTRA_N 12
int amgx_level_extra(amgx_handle h, int level, int64_t* out, int n_out);

/* what amgx_level_desc.jacobi_prec gave this level.  Fills out[0 .. min(n_out, AMGX_JACOBI_PREC_INFO_N)):
 *    0 the passes of this level read float images (0 under AMGX_JACOBI_PREC_F32_WIDE)
 *    1 bit mask of the images converted: A, A', local-window A', diagonal image, Q, local-window Q = bits 0 .. 5
 *    2 value bytes of the float arrays (under AMGX_JACOBI_PREC_F32_WIDE: of the rounded fp64 arrays)
 *    3 fp64 value bytes released
 *    4 the level is the AMGX_JACOBI_PREC_F32_WIDE twin
 * Returns 0, or non-zero for a bad level or n_out < 1. */
#define AMGX_JACOBI_PREC_INFO_N 5
int amgx_jacobi_prec_info(amgx_handle h, int level, int64_t* out, int n_out);

/* what mat_prec = AMGX_PREC_F32_SCALAR_GS gave this level.  Fills out[0 .. min(n_out, AMGX_GS_PREC_INFO_N)):
 *    0 the sweeps of this level read float images (0 under AMGX_GS_F32_WIDE)
 *    1 bit mask of the images converted: A, full, fullLW, lowin, rest, restLW, sell, lower, upper = bits 0 .. 8
 *    2 value bytes of the converted arrays (under AMGX_GS_F32_WIDE: of the rounded fp64 arrays)
 *    3 fp64 value bytes released
 *    4 the level is the AMGX_GS_F32_WIDE twin
 * Returns 0, or non-zero for a bad level or n_out < 1. */
#define AMGX_GS_PREC_INFO_N 5
int amgx_gs_prec_info(amgx_handle h, int level, int64_t* out, int n_out);

/* measurement hook for bench.py: launches one hot-path kernel `reps` times on the handle's stream,
 * bracketed by HIP events, and returns the average duration in milliseconds.
 *   op = 0: residual SpMV  r = b - A_level x      (the dominant kernel of the Jacobi V-cycle)
 *   op = 1: fused Jacobi post-smooth  x' = x + omega*dinv*(b - A_level x)
 *   op = 2: restriction  b_c = P^T r      op = 3: prolongation  x += P x_c
 *   op = 4: one whole cycle (amgx_apply on internal vectors)
 *   op = 5: pre-smoothing + restriction as the V-cycle runs it on this level (fused / folded where built)
 *   op = 6: coarse-grid correction + post-smoothing as the V-cycle runs it on this level
 *   op = 7: sell_pre_restrict_kernel alone (op 5 without the small restrict_sum_kernel); error if the level has none
 *   op = 8: the same kernel timed INSIDE the cycle: `reps` whole cycles are launched directly (no graph) with HIP events
 *           around that one kernel; the average is what rocprofv3 --kernel-trace reports for it (roofline.achieved)
 *   op = 9: like 8 for the backward block-hybrid Gauss-Seidel sweep of the level (gsb_sweep_kernel, the dominant kernel
 *           of a Gauss-Seidel cycle); error if the level has no such sweep
 *   op = 10: one fused Chebyshev step  x' = x + d', d' = c1 d + c2 dinv*(b - A_level x)  (a middle step: d read and stored);
 *           error if the level has no Chebyshev smoother
 *   op = 11: like 9 for the backward Gauss-Seidel sweep of a square-block level (bgsb_sweep_kernel: one launch, or one per block
 *           colour; the launches per colour of the block multicolour forms); error if the level has no block sweep in the cycle.
 *           On a level with single-precision Gauss-Seidel images it reads them
 * ops 5 and 10 time what the cycle runs: on a level with a single-precision image (mat_prec) they read that image; op 0 is
 * amgx_residual's kernel and reads the fp64 image.  On a scalar Jacobi level with jacobi_prec != 0 ops 1, 5, 6, 7 and 8 read the
 * level's single-precision images, on a scalar Gauss-Seidel level with mat_prec = AMGX_PREC_F32_SCALAR_GS ops 5 and 9. */
int amgx_time_op(amgx_handle h, int level, int op, int reps, double* avg_ms);

/* ---- GSS4: Gauss-Seidel on a subset of the rows, on a compressed device copy ------------------------------------------
 * Reference: GSS4<TM> (src/base/smoothers/gssmoother.hpp:99-143, gssmoother.cpp:407-583), the smoother of the EX stage of
 * HybridGSSmoother (gssmoother.cpp:697-698).  Only the rows of the subset are copied to the device ("xdofs" and the
 * compressed matrix cA of GSS4::SetUp, :456-507) together with the transposed couplings the RES form needs.
 *   amgx_gss4_smooth      Smooth (dir 0) / SmoothBack (dir 1):        x_k += dinv_k (b_k - A_k: x)               (:565-583)
 *   amgx_gss4_smooth_res  SmoothRES / SmoothBackRES:  w = -dinv_k res_k; res += A_k:^T w; x_k -= w               (:543-561)
 *   amgx_gss4_mult_add    MultAdd:                                    x_k += s dinv_k b_k  for k in the subset   (:531-539)
 * Rows of equal colour are relaxed in parallel, colours ascending (dir 0) or descending (dir 1); the reference's
 * one-row-at-a-time order is the special case of one row per colour.  Vectors: x and b have A.n_rows * bs entries, except
 * that the gathered vector (x of amgx_gss4_smooth, res of amgx_gss4_smooth_res) has A.n_cols * bs. */
typedef struct amgx_gss4_desc {
  amgx_matrix A;              /* square blocks 1, 2, 3, 6; n_cols >= n_rows (ghost columns are read, never updated)          */
  const uint8_t* subset;      /* [n_rows] 1 = row is smoothed, or NULL (all rows)                                            */
  const double* dinv;         /* [n_rows*bs*bs] inverse of the diagonal block or of its replacement (mod_diag), read on the   */
                              /*   subset only: the caller applies CalcInverse / CalcPseudoInverseTryNormal (:417-438)        */
  const int32_t* color;       /* [n_rows] colour of the rows of the subset (coupled rows differ), -1 elsewhere               */
  int32_t n_colors;
  int32_t device;
} amgx_gss4_desc;
typedef struct amgx_gss4_t* amgx_gss4;

int amgx_gss4_create(const amgx_gss4_desc* desc, amgx_gss4* out);
int amgx_gss4_destroy(amgx_gss4 g);
const char* amgx_gss4_last_error(amgx_gss4 g);            /* g may be NULL for create-time errors */
int amgx_gss4_set_stream(amgx_gss4 g, void* hip_stream);
int amgx_gss4_synchronize(amgx_gss4 g);
/* rows of the subset, rows the subset couples to (= rows of res the RES form updates), blocks stored */
int amgx_gss4_info(amgx_gss4 g, int64_t* n_rows, int64_t* n_touched, int64_t* nnz);
int amgx_gss4_smooth(amgx_gss4 g, int dir, double* x, const double* b, int flags);
int amgx_gss4_smooth_res(amgx_gss4 g, int dir, double* x, double* res, int flags);
int amgx_gss4_mult_add(amgx_gss4 g, double s, const double* b, double* x, int flags);

/* Krylov solvers with all vectors resident on the GPU: the callers of the preconditioner on the
 * reference side are NGSolve's CGSolver / GMRes (tests/h1/amg_utils.py:346).  Operator = the level-0 matrix of the handle,
 * preconditioner = the handle's cycle (use_precond = 0: none).  x holds the initial guess and receives the solution.
 *   amgx_pcg  : err_k = sqrt(|<C r_k, r_k>|), stops at err_k <= tol * err_0 (CGSolver's criterion)
 *   amgx_gmres: restarted GMRES(restart), left-preconditioned, err_k = |C r_k|
 * errs (optional, maxit + 1 entries) receives err_0 ... err_iters; *iters (optional) the iteration count.  BLAS-1 work runs in
 * hand-written kernels with deterministic reductions; the host reads one scalar per iteration.
 * Edges: err_0 == 0 returns at once with 0 iterations.  amgx_pcg tests its criterion after an iteration, amgx_gmres before a restart
 * cycle as well: tol >= 1 gives 1 PCG iteration and 0 GMRES iterations.  maxit = 0 leaves x as it is; amgx_pcg then still writes
 * errs[0] = err_0, amgx_gmres (which computes err_0 inside its first cycle) does not touch errs.  maxit counts iterations over all
 * restart cycles: a cycle cut short by maxit still updates x.  1 <= restart <= 40; a larger value is an error ("restart lengths
 * above 40 are not supported"), restart > maxit is allowed.  AMGX_PCG_SINGLE_REDUCTION with use_precond = 0 runs the classical form. */
int amgx_pcg(amgx_handle h, const double* b, double* x, double tol, int maxit, int use_precond, int flags, double* errs, int32_t* iters);
int amgx_gmres(amgx_handle h, const double* b, double* x, double tol, int maxit, int restart, int use_precond, int flags, double* errs,
               int32_t* iters);

/* ---- multi-vectors: k right-hand sides per matrix pass -------------------------------------------------------------------
 * Reference interface: BaseMatrix::Mult / MultAdd on an NGSolve MultiVector (the block of vectors of LOBPCG / PINVIT, several
 * load cases for one operator); the reference applies AMGMatrix::Mult (amg_matrix.cpp:377-378) once per vector.  1 <= k <=
 * AMGX_MULTI_MAX; layout by AMGX_MULTI_INTERLEAVED, host / device pointers and AMGX_NO_GRAPH as in amgx_apply.
 *   amgx_apply_multi : column j of X = C (column j of B), the operator of amgx_apply; k = 1 IS amgx_apply
 *   amgx_matvec_multi: column j of Y = A_level (column j of X)   (GetMatrix(level).Mult per vector)
 *   amgx_pcg_multi   : k INDEPENDENT recurrences of amgx_pcg (not block CG) that share the level-0 product and the
 *                      preconditioner application; per column err_k = sqrt(|<C r_k, r_k>|), stop at err_k <= tol * err_0.  A column
 *                      that has met its criterion (or has err_0 == 0) is frozen: its x is not touched again, iters[j] is the
 *                      iteration at which it stopped; the call returns when every column is frozen or at maxit.  errs (optional,
 *                      k rows of maxit + 1 entries): row j holds err_0 .. err_iters[j] of column j.  iters: [k], required.  The
 *                      host reads k scalars per iteration in one copy.  (AMGX_PCG_SINGLE_REDUCTION is ignored: classical form.)
 * A handle whose smoothed levels are all scalar (1x1), plain Jacobi (sm_steps = 1, no sm_symm), square, and whose cycle is V runs
 * FUSED: the literal cycle (x = w Dinv b, r = b - A x, b_c = P^T r, ..., t = x + P x_c, x = t + w Dinv (b - A t)) on A, P, P^T with
 * every matrix entry read once for 2 or 4 interleaved vectors; any other k is cut greedily into groups of those widths (8 = 4 + 4:
 * a width-8 kernel measured slower per column) plus at most one single column, which takes the single-vector path.  Every other handle (Gauss-Seidel in any form, Chebyshev, block levels, W / BS
 * cycles, ProxySmoother) answers the same calls through a column loop over the single-vector path -- all or nothing per handle.
 *   amgx_multi_info  : fused = 1 / 0 as above; the groups a call with k columns runs as (group_width: AMGX_MULTI_MAX entries,
 *                      0 beyond n_groups; all 1 when fused = 0); work_bytes = device memory of the multi-vector work space such a
 *                      call allocates (kept until amgx_destroy).  Any of the output pointers may be NULL.
 * With AMGX_MULTI_FUSE the rule is wider (opt-in per call): V cycle; every level square and in the caller's
 * numbering; every smoothed level plain (sm_steps = 1, no sm_symm) with AMGX_SM_JACOBI or AMGX_SM_CHEBY, mixed freely from level to
 * level; block size 1, 2, 3 or 6; A in SELL (plain or windowed), CSR-vector, BSELL or block CSR with a square block; P, P^T scalar,
 * rigid-body transfer blocks or block CSR (22, 33, 66, 36, 63, 23, 32).  Chebyshev levels run the literal recurrence of the
 * single-vector smoother with the same coefficients and read the single-precision image where the level has one; amgx_matvec_multi
 * and the level-0 product of amgx_pcg_multi read the fp64 image.  Gauss-Seidel in any form, W / BS cycles and the ProxySmoother keep
 * the column loop.
 * With AMGX_MULTI_FUSE_GS (opt-in per call; it implies AMGX_MULTI_FUSE) a smoothed level may also be AMGX_SM_GS,
 * mixed freely with Jacobi and Chebyshev levels, if it is scalar (bs = 1), square, in the caller's numbering, plain, and swept in
 * the block-hybrid or the scalar multicolour form.  Its sweeps keep, per column, the order of additions of the single-vector
 * sweep: a column of amgx_smooth_multi equals amgx_smooth bit for bit.  Gauss-Seidel on a block level and AMGX_SM_BGS keep the
 * column loop (amgx_multi_note names the smoother and the level).  So does a handle with a Gauss-Seidel level that reads
 * single-precision images (mat_prec = AMGX_PREC_F32): the fused sweeps read fp64 images, and the note says "single-precision
 * Gauss-Seidel images (level l)".
 * A handle with a scalar Gauss-Seidel level that has single-precision images (mat_prec = AMGX_PREC_F32_SCALAR_GS; the
 * AMGX_GS_F32_WIDE twin too) is not fused under AMGX_MULTI_FUSE_GS / _GS_BLOCK with the same note, and amgx_smooth_multi, amgx_down_multi
 * and the two _DOWN bits keep the column loop on such a level: the fp64 values of its sweep images are released.
 * A handle with a scalar Jacobi level that reads single-precision images (jacobi_prec != 0) is not fused under any
 * of these flags, the default rule included, and amgx_down_multi keeps the column loop on such a level: the multi-vector kernels read
 * fp64 images.  The note says "single-precision Jacobi images (level l)"; a column equals amgx_apply bit for bit.
 * With AMGX_MULTI_FUSE_GS_BLOCK (opt-in per call; it implies the two flags above) an AMGX_SM_GS level may also have
 * block size 2, 3 or 6, if it is square, in the caller's numbering, plain, and swept in the hybrid-block, the block-coloured, the
 * multicolour BSELL or the multicolour row-list form (compact sweep blocks, gs_block_ids, included), and if its sweep block fits
 * 64 KB of LDS on 4 vectors (2 * gs_block_rows * bs * 4 doubles + the row ids; every default block does, otherwise the note is
 * "sweep block too large for the multi-vector sweep (level l)").  Per column the sweeps keep the order of additions of the
 * single-vector kernels at the default AMGX_BSELL_XMODE: a column of amgx_smooth_multi equals amgx_smooth bit for bit there too.
 * AMGX_SM_BGS, W / BS cycles, sm_steps > 1 / sm_symm (ProxySmoother) and rank-partitioned levels keep the column loop, each with a
 * note of its own; so do groups wider than 4.
 *   amgx_smooth_multi: one plain smoother step per column, amgx_smooth(level, dir, x_j, b_j, res, 0, 0, x_zero) with a res of its
 *                      own; layout and pointers as in amgx_matvec_multi, X and B have the level's size (no ghost entries).  With
 *                      AMGX_MULTI_FUSE_GS on a Gauss-Seidel level that has the multi-vector sweep, groups of 4 and 2 columns run it
 *                      (whatever the rest of the handle looks like; a square-block level needs AMGX_MULTI_FUSE_GS_BLOCK); otherwise, and for a single left-over column, a column loop
 *                      over the single-vector step.  x_zero is the caller's promise that X is zero, as in amgx_smooth.
 *   amgx_multi_plan  : the outputs of amgx_multi_info for a call that carries `flags` (only AMGX_MULTI_FUSE, AMGX_MULTI_FUSE_GS and
 *                      AMGX_MULTI_FUSE_GS_BLOCK are looked at; flags = 0 answers exactly what amgx_multi_info answers); work_bytes counts one more vector per
 *                      Chebyshev level
 *   amgx_multi_note  : the first reason why the handle is not fused under `flags` (it names the level), "" when it is fused.  The
 *                      string lives until the calling thread's next amgx_multi_note
 * With AMGX_MULTI_FUSE_DOWN = 512 (opt-in per call; it implies nothing and modifies whichever fused cycle the other
 * flags select, the default fused Jacobi handle with no other flag included) a fused group of 2 or 4 columns runs the down pass of
 * every smoothed scalar level that qualifies as the single-vector cycle does: r = b - A x formed in LDS, the chunk-local P^T r taken
 * from there, then the sum of the partial sums -- instead of writing r, gathering it through P^T and, on Jacobi levels, the separate
 * x = w Dinv b.  A level qualifies if the single-vector cycle has the fused down launch for its smoother (Jacobi from zero, the
 * residual after Chebyshev, the residual after a block-hybrid Gauss-Seidel sweep from zero), the launch reads a plain SELL image
 * (or, after a Gauss-Seidel sweep, a windowed one) with 512-lane workgroups, and one lane per row with 4 or 6 entries of P per
 * thread or 2 / 4 / 8 lanes with 4.  A Jacobi level that qualifies and has the folded prolongation Q in a SELL / CSR-vector form
 * also runs the way up as x = z + Q x_c.  Every other level keeps the literal stages (local-window and diagonal images, other
 * workgroup sizes, levels without the chunk-local restriction, block levels, the multicolour sweep); mixing per level is allowed.
 * Per column the kernels keep the order of additions of the single-vector kernels: a column of amgx_down_multi is the same with
 * and without the bit, bit for bit.  The column loop and k = 1 ignore the bit; amgx_multi_plan counts the partial-sum buffers.
 * With AMGX_MULTI_FUSE_DOWN_DIA = 1024 (opt-in per call; it implies AMGX_MULTI_FUSE_DOWN and nothing else, and is
 * looked at by amgx_multi_plan, amgx_multi_note, amgx_multi_level_plan, amgx_multi_level_note, amgx_down_multi, amgx_apply_multi and
 * amgx_pcg_multi) a level whose fused Jacobi down launch reads the symmetric diagonal image qualifies too, with 512-row chunks (1 .. 8
 * upper diagonals, 4 or 6 entries of P per thread: form "dia") and with box chunks of grid lines (2 .. 7 upper diagonals: form
 * "dia-box", dynamic LDS of 8 * (box rows * NV + max(box rows * NV, entries of the fullest box)) bytes, at most 160 KB).  The fold rule
 * is relaxed as well: a Jacobi level that takes a fused down pass under this flag runs the way up as x = z + Q x_c on the plain
 * windowed Q even where the single-vector cycle runs the local-window image of Q.  Levels with a local-window image of A' keep the
 * note "local-window image".  Under AMGX_MULTI_FUSE_DOWN alone "diagonal image" remains the note of such a level and the fold rule is
 * the one above; the column loop and k = 1 ignore the flag like its neighbours.  A column of amgx_down_multi is the same with and
 * without it, bit for bit.
 * With AMGX_MULTI_FUSE_F32 = 2048 (opt-in per call; it implies nothing, is never an error and is looked at wherever
 * AMGX_MULTI_FUSE_GS is: amgx_apply_multi, amgx_pcg_multi, amgx_smooth_multi, amgx_multi_plan / amgx_multi_note, amgx_down_multi,
 * amgx_multi_level_plan / amgx_multi_level_note) a Gauss-Seidel level with single-precision images is admitted by the rule of
 * AMGX_MULTI_FUSE_GS (scalar levels, mat_prec = AMGX_PREC_F32_SCALAR_GS) or AMGX_MULTI_FUSE_GS_BLOCK (2x2 / 3x3 / 6x6 levels, mat_prec =
 * AMGX_PREC_F32), which must be carried too.  The AMGX_GS_F32_WIDE twins are admitted by the same flag and run the fp64
 * multi-vector kernels on their rounded values.  What a fused group of such a handle runs, stated once:
 *   fused on 2 or 4 columns, reading the float arrays the single-vector passes read with their order of additions per column
 *   (a column of amgx_smooth_multi equals amgx_smooth bit for bit): every Gauss-Seidel sweep, the sweep from zero included; the
 *   residual after the sweep from zero where it is a product of its own on a sliced-ELL or BSELL image (`rest`, `upper` / `bupper`,
 *   or A of a level without the split images); the transfers of scalar levels.
 *   per column through the single-vector kernels, because the single-vector cycle is not the literal cycle there: the levels of the
 *   single-workgroup coarse tail (which reads true fp64 copies of A); the residual that is fused with the chunk-local restriction
 *   after a block-hybrid sweep from zero on a scalar level; on 2x2 / 3x3 / 6x6 levels the transfers P^T and P, the coarsest solve, and
 *   the residual of a level without the split images whose A is block CSR (block-CSR products on one and on 2 / 4 vectors add in
 *   different orders).
 * So a column of amgx_apply_multi equals amgx_apply bit for bit, up to the dense product of a collapsed coarse tail.
 * A level qualifies if every image its fused passes read has a multi-vector kernel on the array the single-vector pass reads: float
 * arrays of the sliced-ELL / BSELL sweep images, of `rest` (plain or windowed sliced-ELL, BSELL) and of A (plain sliced-ELL, BSELL)
 * on a level without the split images; an image in a format without a float kernel (CSR-vector `rest`, windowed or CSR A) keeps its
 * rounded values at fp64 width, which both paths read.  A level that does not qualify keeps the note "single-precision Gauss-Seidel
 * images (level l)"; so does every such level without the flag.  "single-precision Jacobi images" stays a refusal under every flag,
 * and on a handle without such Gauss-Seidel levels the flag changes nothing.  The two _DOWN bits still keep the literal stages on
 * such a level (amgx_multi_level_note: "single-precision Gauss-Seidel images"); amgx_down_multi with x_given = 0 under
 * AMGX_MULTI_FUSE_DOWN | AMGX_MULTI_FUSE_GS | AMGX_MULTI_FUSE_F32 runs the multi-vector float sweep from zero on groups of 4 and 2
 * columns and then the single-vector residual and restriction per column.
 * With AMGX_MULTI_FUSE_DOWN_F32 = 4096 (opt-in per call; it implies AMGX_MULTI_FUSE_DOWN and AMGX_MULTI_FUSE_F32 and
 * nothing else, is never an error and is looked at wherever AMGX_MULTI_FUSE_DOWN is) the refusal "single-precision Gauss-Seidel
 * images" of the down pass is lifted for a scalar level whose single-vector cycle fuses the residual after the block-hybrid sweep from
 * zero with the chunk-local restriction, where the level qualifies under AMGX_MULTI_FUSE_F32 and the image that launch reads has the
 * array the single-vector launch reads (the float array; on the AMGX_GS_F32_WIDE twin the rounded values at fp64 width).  The forms:
 * "sell" and "sell-win" as under AMGX_MULTI_FUSE_DOWN, on the float array; and, under this flag alone, "sell-lw" (form 5), the
 * local-window image of `rest` with 2 or 4 lanes per row and 2 or 4 entries of P per thread, where both widths fit
 * 8 * (W * NV + (512 / lanes) * NV + EPT * 512) bytes of dynamic LDS in 160 KB (W: the longest column list of the level's chunks);
 * otherwise the level keeps the note "local-window image".  A fused group then runs the multi-vector float sweep from zero and this
 * launch instead of k single-vector residual + restriction passes; per column the kernels keep the order of additions of the
 * single-vector float kernels, so a column of amgx_down_multi and of amgx_apply_multi is the same with and without the flag, bit for
 * bit.  On a handle without single-precision Gauss-Seidel images the flag changes nothing beyond AMGX_MULTI_FUSE_DOWN |
 * AMGX_MULTI_FUSE_F32 (levels with a local-window image on fp64 handles keep their note); "single-precision Jacobi images",
 * "multicolour sweep", "block level" and "workgroup size" stay refusals.
 *   amgx_down_multi  : the down stage of a level per column; layout and pointers as in amgx_matvec_multi; B and X have the level's
 *                      size, BC the coarse level's.  The level must be scalar and smoothed, without ghost columns and not
 *                      renumbered.  x_given = 0: X is output -- pre-smoothing from zero, then b_c = P^T (b - A x), the down stage of
 *                      the single-vector V-cycle (X holds z = x + w Dinv r on a level with the folded prolongation).  x_given = 1:
 *                      X is input, the iterate after the level's pre-smoothing, and only the residual + restriction half runs (on a
 *                      Jacobi level with a fused down launch that is an error: the Jacobi down pass forms x itself).  Without
 *                      AMGX_MULTI_FUSE_DOWN a column loop over the single-vector functions; with it groups of 4 and 2 columns run
 *                      the multi-vector kernels where the level qualifies (a Gauss-Seidel level with x_given = 0 also needs
 *                      AMGX_MULTI_FUSE_GS for its sweep), and a left-over column takes the single-vector path.
 *   amgx_multi_level_plan: out[0 .. 4] = the down form of the level under `flags` (0 literal, 1 sell, 2 windowed sell; with AMGX_MULTI_FUSE_DOWN_DIA
 *                      also 3 diagonal image on 512-row chunks, 4 diagonal image on box chunks; with AMGX_MULTI_FUSE_DOWN_F32 also 5
 *                      local-window image), the mode
 *                      (0 Jacobi from zero, 1 after a block-hybrid sweep, 2 after Chebyshev), folded way up (0 / 1), single-precision
 *                      image (0 / 1), bytes of LDS of a workgroup on 4 vectors.  All 0 without AMGX_MULTI_FUSE_DOWN.
 *   amgx_multi_level_note: why the level stays literal under `flags`: "local-window image", "diagonal image", "workgroup size",
 *                      "no chunk-local restriction", "block level", "multicolour sweep" ("windowed image": the windowed image of A' behind
 *                      the AMGX_APRE_WINDOW A/B hook); "" when it does not (or without the bit).
 *                      The string lives until the calling thread's next amgx_multi_level_note */
#define AMGX_MULTI_MAX 8
int amgx_apply_multi(amgx_handle h, int k, const double* B, int64_t ldb, double* X, int64_t ldx, int b_status, int flags);
int amgx_matvec_multi(amgx_handle h, int level, int k, const double* X, int64_t ldx, double* Y, int64_t ldy, int flags);
int amgx_pcg_multi(amgx_handle h, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double tol, int maxit, int use_precond, int flags,
                   double* errs, int32_t* iters);
int amgx_smooth_multi(amgx_handle h, int level, int dir, int k, double* X, int64_t ldx, const double* B, int64_t ldb, int x_zero, int flags);
int amgx_multi_info(amgx_handle h, int k, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes);
int amgx_multi_plan(amgx_handle h, int k, int flags, int32_t* fused, int32_t* n_groups, int32_t* group_width, int64_t* work_bytes);
const char* amgx_multi_note(amgx_handle h, int flags);
int amgx_down_multi(amgx_handle h, int level, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double* BC, int64_t ldbc, int x_given,
                    int flags);
int amgx_multi_level_plan(amgx_handle h, int level, int flags, int32_t* out, int n_out);
const char* amgx_multi_level_note(amgx_handle h, int level, int flags);

/* ---- multi-vector algebra: Gram matrices and combinations -------------------------------------------------------------------
 * Reference interface: NGSolve's MultiVector.InnerProduct (the small matrices X^T Y of a Rayleigh-Ritz step) and
 * MultiVector * matrix (the updates Y <- X c) -- with amgx_matvec_multi and amgx_apply_multi the four operations of the LOBPCG /
 * PINVIT loops of ngsolve.eigenvalues (a Python loop there, ngsamg_amd.eigen here).  The handle gives the device, the stream,
 * the error slot and the work space (kept until amgx_destroy); n is free, it need not be a level size.  Vectors: host or device
 * pointers by AMGX_HOST_PTR / AMGX_DEVICE_PTR; layout column-major with ld >= n, or with AMGX_MULTI_INTERLEAVED entry (row, column
 * j) at row*k + j and ld ignored.  The small matrices G and c are ALWAYS host arrays, row-major.  1 <= k <= AMGX_MV_MAX on every
 * side.  Errors: k out of range, ld < n without the interleaved flag, a null pointer with n > 0, n < 0.
 *   amgx_mv_gram   : G[i*kb + j] = <A_i, B_j>.  One pass over the vectors (8 n (ka + kb) bytes), any ka, kb: row chunks of all
 *                    columns are staged in LDS and multiplied by v_mfma_f64_16x16x4_f64.  Deterministic: per-workgroup partial
 *                    sums from a launch shape that depends on (n, ka, kb, layout) only (amgx_mv_gram_plan reports it), final
 *                    sums by a second launch in a fixed order, no atomics: two calls on the same data return the same bits.
 *                    A == B with lda == ldb and ka == kb: only the upper triangle is computed (8 n ka bytes) and mirrored, G is
 *                    symmetric bit for bit.  Synchronises the stream before it returns (the caller needs G).  n = 0: G = 0.
 *   amgx_mv_combine: Y_j = beta*Y_j + sum_i c[i*ky + j] X_i, per entry beta*y first, then i ascending, fused multiply-add;
 *                    8 n (kx + ky (1 + [beta != 0])) bytes.  beta == 0: Y is not read (NaNs in it do not propagate).  Y must not
 *                    be one of the X arrays: the same base pointer is an error.  c travels through a small ring of device
 *                    buffers: with device vectors nothing synchronises the host.  n = 0 returns at once.
 *   amgx_mv_gram_plan: rows of one staged chunk and workgroups of amgx_mv_gram for these sizes (symmetric: the A == B form) */
#define AMGX_MV_MAX 32
int amgx_mv_gram(amgx_handle h, int64_t n, int ka, const double* A, int64_t lda, int kb, const double* B, int64_t ldb, double* G, int flags);
int amgx_mv_combine(amgx_handle h, int64_t n, int kx, const double* X, int64_t ldx, const double* c, int ky, double beta, double* Y, int64_t ldy,
                    int flags);
int amgx_mv_gram_plan(amgx_handle h, int64_t n, int ka, int kb, int symmetric, int32_t* chunk_rows, int32_t* n_blocks);

/* ------------------------------------------------------------------------------------------------------------------
 * Rank-partitioned hierarchies (one process per GPU; SURVEY.md 8b "halo tables + RCCL communicator", 8e).
 *
 * What the reference does with MPI -- every rank of the communicator calls AMGMatrix::Mult collectively
 * (src/base/solve/amg_matrix.cpp:160-307), smoothers exchange halos through DCCMap (src/base/linalg/dcc_map.cpp:17-302)
 * around their local stages (src/base/smoothers/hybrid_base_smoother.cpp:501-574) -- is one call here: amgx_dist_apply.
 * Layout: a rank stores the rows of the vertices it owns, columns [owned | ghost], ghosts grouped by owning rank
 * (ascending), owned rows ordered [interior | boundary] (interior = no ghost column).  Pack kernels + ncclSend / ncclRecv
 * run on a communication stream while the interior rows are processed; nothing synchronises the host.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct amgx_comm_t* amgx_comm;
typedef struct amgx_dist_t* amgx_dist;
typedef struct amgx_halo_t* amgx_halo;
enum {
  AMGX_COMM_RCCL = 0,         /* one rank per process, ncclCommInitRank over xGMI (replaces the MPI communicator)          */
  AMGX_COMM_LOCAL = 1         /* all n_ranks ranks live in this process on one GPU ("virtual ranks": tests, rehearsal);     */
                              /*   same kernels, streams and events, device copies instead of ncclSend / ncclRecv           */
};
#define AMGX_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: called by rank 0, the caller distributes the 128 bytes (e.g. torch.distributed / MPI_Bcast) */
int amgx_comm_unique_id(char* id128);
/* RCCL: collective over all ranks (ncclCommInitRank); LOCAL: rank and id128 are ignored */
int amgx_comm_create(int kind, int n_ranks, int rank, const char* id128, int device, amgx_comm* out);
int amgx_comm_destroy(amgx_comm c);                      /* also destroys the hierarchies created on it */
const char* amgx_comm_last_error(amgx_comm c);           /* c may be NULL for create-time errors        */
/* compute stream of the communicator (and of every hierarchy on it); NULL = its own stream */
int amgx_comm_set_stream(amgx_comm c, void* hip_stream);
int amgx_comm_synchronize(amgx_comm c);
int amgx_comm_info(amgx_comm c, int32_t* kind, int32_t* n_ranks, int32_t* rank, int64_t* n_exchanges);
/* how amgx_dist_apply launches (no reference counterpart: the reference's cycle is a host loop around MPI calls,
 * amg_matrix.cpp:160-307 / dcc_map.cpp:76-178): with device vectors the whole collective cycle -- both streams, pack kernels,
 * ncclSend / ncclRecv / ncclAllGather -- is captured once per (b, x, b_status) into a hipGraph and replayed.  enabled = 0
 * after AMGX_DIST_GRAPH=0 or a failed capture (note: why; direct launches from then on); n_graphs = captured cycles held,
 * n_replays = applications served by a graph launch. */
int amgx_comm_graph_info(amgx_comm c, int32_t* enabled, int64_t* n_graphs, int64_t* n_replays);
/* how directly launched work on the compute and the communication stream is ordered: event_order = 1 events (hipEventRecord /
 * hipStreamWaitEvent: AMGX_DIST_EVENTS=1 at amgx_comm_create, or a device without stream memory operations), 0 device flags
 * (hipStreamWriteValue64 / hipStreamWaitValue64).  Inside a captured graph the order is always a graph edge. */
int amgx_comm_order_info(amgx_comm c, int32_t* event_order);
const char* amgx_comm_graph_note(amgx_comm c);

/* halo tables of one level = DCCMap's m_ex_dofs / g_ex_dofs (dcc_map.cpp:480-543) in owner-row form */
typedef struct amgx_halo_desc {
  int32_t n_peers;
  const int32_t* peer_rank;   /* [n_peers] ascending (GetDistantProcs)                                              */
  const int64_t* send_ptr;    /* [n_peers+1]                                                                        */
  const int32_t* send_idx;    /* owned block rows whose values peer k ghosts (m_ex_dofs[k]), in the order of the     */
                              /*   peer's ghost segment                                                              */
  const int64_t* recv_ptr;    /* [n_peers+1] ghost block rows [recv_ptr[k], recv_ptr[k+1]) belong to peer k           */
                              /*   (g_ex_dofs[k]; contiguous: ghosts are grouped by owner)                           */
  int64_t n_interior;         /* owned rows [0, n_interior) have no ghost column (split_ind analogue,                 */
                              /*   gssmoother.cpp:664-678); 0 = no overlap of communication and computation          */
} amgx_halo_desc;

typedef struct amgx_dist_desc {
  amgx_hierarchy_desc top;    /* levels 0..k of this rank: A = owned rows x [owned | ghost]; P, PT rank-local; Jacobi   */
                              /*   levels with fold: Q (columns = coarse [owned | ghost]); dinv / colours / blocks as    */
                              /*   usual (dinv over n_cols entries for Jacobi and Chebyshev); level k: only A (its shape */
                              /*   is used).  AMGX_SM_CHEBY levels: one cheb_degree and cheb_ratio on all of them, fp64  */
                              /*   storage (mat_prec = AMGX_PREC_F32 is refused), no fold; cheb_lambda_max = 0: see      */
                              /*   amgx_dist_cheb_estimate.  The replicated tail may use AMGX_SM_CHEBY as any handle.    */
                              /*   Both need amgx_dist_desc.cheby = 1                                                    */
  const amgx_halo_desc* halo; /* [k] halo tables of the levels 0..k-1                                                    */
  amgx_hierarchy_desc tail;   /* replicated coarse hierarchy; its level 0 = level k gathered in rank order (CtrMap,      */
                              /*   src/base/coarsening/dof_contract.cpp:49-223, without the hop back)                    */
  const int64_t* counts;      /* [n_ranks] owned block rows of level k per rank                                          */
  const int64_t* kmap;        /* [kmap_len] level-k [owned | ghost] scalar entries -> scalar index in the gathered vector */
  int64_t kmap_len;
  int32_t rank;               /* this rank (LOCAL communicators: ranks are created in order 0, 1, ...)                   */
  int32_t fold;               /* Jacobi: 1 = post-smoothing folded into the prolongation (2k-1 exchanges), 0 = literal   */
  const int32_t* gs_stage;    /* optional [4*k]: colour ranges of the hybrid Gauss-Seidel stages per level,              */
                              /*   [s0,s1) first local part, [s1,s2) rows that read ghosts ("EX"), [s2,s3) second local   */
                              /*   part (gssmoother.cpp:721-782); NULL: one stage                                        */
  int32_t cheby;              /* opt-in, like AMGX_MULTI_FUSE: 1 = the caller asks for AMGX_SM_CHEBY levels in `top` /    */
                              /*   `tail` (an own option beyond the reference; 2 x cheb_degree halo exchanges per level   */
                              /*   and application).  0: a descriptor with such a level is refused, as it always was      */
} amgx_dist_desc;

int amgx_dist_create(amgx_comm c, const amgx_dist_desc* desc, amgx_dist* out);
int amgx_dist_destroy(amgx_dist d);
/* x = C b collectively.  b, x: one pointer per local rank (RCCL: one).  b_status 1 (CUMULATED): b holds the owned entries;
 * 0 (DISTRIBUTED): b holds [owned | ghost] entries whose ghost part are contributions to the owners, added first
 * (b.Distribute() state, amg_matrix.cpp:164; DCCMap DIS2CO).  x: owned entries (CUMULATED on the owners).
 * flags: AMGX_HOST_PTR / AMGX_DEVICE_PTR. */
int amgx_dist_apply(amgx_comm c, const double* const* b, double* const* x, int b_status, int flags);
/* lambda_max(Dinv A) of the rank-partitioned AMGX_SM_CHEBY levels created with cheb_lambda_max = 0: the estimator of amgx_create
 * (30 power steps, 1.1 x the last Rayleigh quotient) on the partitioned operator.  Start vector: the deterministic fill at every
 * rank's LOCAL scalar index; an owner -> ghost exchange ahead of every product; the two inner products per step are deterministic
 * local reductions + one all-reduce of two scalars, and every rank decides on the reduced values: all ranks end with bitwise the
 * same interval, hence the same coefficients.  Collective (it cannot run inside amgx_dist_create: local ranks are created one by
 * one); idempotent; a no-op when nothing is to be estimated.  amgx_dist_apply / _pcg / _gmres / _time_kernel call it first if it
 * has not run.  Afterwards amgx_smoother_info on the borrowed top handle answers estimated = 1. */
int amgx_dist_cheb_estimate(amgx_comm c);
/* Preconditioned CG on the rank-partitioned level-0 operator, collectively (the reference's driver: NGSolve CGSolver on
 * ParallelVectors, tests/h1/amg_utils.py:337-363, whose inner products are MPI all-reduces): level-0 product with one owner ->
 * ghost exchange behind the interior rows, preconditioner = amgx_dist_apply (replayed from its graph), the two inner products
 * per iteration are deterministic local reductions + one ncclAllReduce of a device scalar each, recurrence scalars stay on the
 * device, every rank reads the same error value and takes the same decision.  b, x: device pointers to the OWNED entries, one
 * per local rank; x holds the initial guess.  err_k, tol, errs, iters as amgx_pcg. */
int amgx_dist_pcg(amgx_comm c, const double* const* b, double* const* x, double tol, int maxit, int use_precond, int flags, double* errs,
                  int32_t* iters);
/* Restarted GMRES(restart), left-preconditioned, on the rank-partitioned level-0 operator, collectively (reference driver:
 * ngsolve.krylovspace.GMRes on ParallelVectors): Arnoldi inner products = one fused local pass + one ncclAllReduce of j + 1
 * scalars per Gram-Schmidt pass, Givens rotations on every rank alike.  Arguments as amgx_dist_pcg / amgx_gmres. */
int amgx_dist_gmres(amgx_comm c, const double* const* b, double* const* x, double tol, int maxit, int restart, int use_precond, int flags,
                    double* errs, int32_t* iters);
/* Measurement hook, collective (every rank calls it with the same arguments): `reps` whole cycles with direct launches, HIP
 * events around ONE kernel of the first local rank's level `level` -- op 8: the fused Jacobi pre-smoothing + residual +
 * restriction kernel over the INTERIOR rows (the launch that runs beside the halo exchange); op 9: the backward block-hybrid
 * Gauss-Seidel sweep over the interior blocks.  The counterpart of amgx_time_op(op 8 / 9) for rank-partitioned hierarchies:
 * the kernel is timed where it runs, with the exchange in flight next to it. */
int amgx_dist_time_kernel(amgx_comm c, int level, int op, int reps, double* avg_ms);
/* the level-0 right-hand-side buffer of a rank ([owned | ghost], device): filling it in place saves the copy of b */
int amgx_dist_rhs_buffer(amgx_dist d, double** b, int64_t* n_owned, int64_t* n_ext);
/* borrowed handles of the rank-partitioned levels and of the replicated tail, for queries / measurement only */
int amgx_dist_handles(amgx_dist d, amgx_handle* top, amgx_handle* tail);

/* ---- setup products on the device (cold path; host arrays in, host arrays out) ---------------------------------------------
 * C = A B (MatMultABImpl, src/base/linalg/utils_sparseMM.cpp:107-238) and the Galerkin product A_c = (P^T A) P
 * (RestrictMatrix, utils_sparseMM.hpp:93-109; the intermediate P^T A stays on the device) for (block-)CSR matrices (result blocks
 * of at most 36 entries: 1x1 ... 6x6), columns ascending per row.  Entry (i, j) is accumulated as c = fma(a_ik, b_kj, c) over k
 * ascending from c = 0 (blocks: c[r][s] = fma(a[r][q], b[q][s], c[r][s]), q ascending inside every block product) -- the order and
 * the fused multiply-add of the host library's product (csrc/host/sparse.cpp), so the result is the same bit for bit.
 * Returns 0 = done (*out holds the result on the device, *n_rows / *nnz its size in block rows / blocks: allocate and call
 * amgx_csr_result_fetch, which copies the arrays out and releases the result), 2 = not supported (larger blocks, a row with more
 * than 8192 products or, block matrices, more distinct columns than one wave's table holds): the caller keeps its own product,
 * 1 = error (amgx_last_error(NULL)).
 * The host setup library takes the pair (amgx_galerkin, amgx_csr_result_fetch) through amgh_set_galerkin_hook (amgh.h). */
typedef struct amgx_csr_result_t* amgx_csr_result;
int amgx_device_count(int32_t* n);      /* visible HIP devices (0 without a GPU or driver; never an error) */
int amgx_spgemm(const amgx_matrix* A, const amgx_matrix* B, amgx_csr_result* out, int64_t* n_rows, int64_t* nnz);
int amgx_galerkin(const amgx_matrix* PT, const amgx_matrix* A, const amgx_matrix* P, amgx_csr_result* out, int64_t* n_rows, int64_t* nnz);
int amgx_csr_result_fetch(amgx_csr_result res, int64_t* rowptr, int32_t* col, double* val);

/* stand-alone halo map = DCCMap (dcc_map.hpp:20-90): mode 0 owner -> ghost overwrite (StartCO2CU / ApplyCO2CU,
 * dcc_map.cpp:138-178), mode 1 ghost -> owner add with the ghost entries zeroed (StartDIS2CO / ApplyDIS2CO, :76-136).
 * vecs: device vectors of (n_owned + n_ghost) * bs entries, ordered on the communicator's stream. */
int amgx_halo_create(amgx_comm c, const amgx_halo_desc* d, int64_t n_owned, int64_t n_ghost, int32_t bs, int32_t rank, amgx_halo* out);
int amgx_halo_destroy(amgx_halo h);
int amgx_halo_exchange(amgx_comm c, int n_local, const amgx_halo* halos, double* const* vecs, int mode);

#ifdef __cplusplus
}
#endif
#endif
