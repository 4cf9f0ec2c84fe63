/*
 * lkamd.h -- C ABI of the MI355X (gfx950) backend for LensKit's hot path.
 *
 * Every entry point replaces one function of the reference's native module
 * `lenskit._accel` (Rust/PyO3) or the NumPy call next to it; the reference
 * interface each one stands in for is cited as file:line relative to the
 * lenskit/lkpy checkout.  Plain pointers and sizes only: no torch / Arrow /
 * Python types cross this boundary.  INTEGRATION.md shows the binding a
 * LensKit maintainer would add on the reference side.
 *
 * Conventions
 *  - `d_` pointers are DEVICE pointers (HBM); `h_` pointers are HOST pointers.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *    device entry points are asynchronous on that stream unless stated.
 *  - Return value: 0 on success, negative LK_E_* code on failure;
 *    lk_last_error() returns a thread-local message for the last failure.
 *  - CSR: `indptr` has n_rows+1 entries, int32 or int64 (`indptr_is_64`);
 *    `indices` int32; `values` float32.  This is the layout of the
 *    reference's SparseRowArray (src/lenskit/data/matrix.py:318-539; Rust view
 *    src/accel/sparse/csr.rs:44-223): Arrow List<Struct{index:i32,value:f32}>
 *    (int32 offsets) or LargeList (int64 offsets).
 *  - Factor matrices are row-major float32 with an explicit leading dimension
 *    `ld` (floats).  The kernels require ld == lk_padded_dim(k) and the pad
 *    columns [k, ld) to be zero; lk_pad_rows / lk_unpad_rows convert.
 */
#ifndef LKAMD_H
#define LKAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_OK 0
#define LK_E_INVALID (-1)   /* bad argument (shape, k, null pointer) */
#define LK_E_HIP (-2)       /* HIP runtime error */
#define LK_E_NOT_SPD (-3)   /* ALS normal matrix not positive definite
                               (reference: RuntimeError("ALS solve error: ..."),
                               src/accel/als/implicit.rs:79, solve.rs:99-105) */
#define LK_E_NAN_SIM (-4)   /* NaN similarity (reference: ValueError("similarity is
                               null"), src/accel/knn/accum.rs:146-151) */
#define LK_E_NOMEM (-5)
#define LK_E_CANCELLED (-6) /* cooperative cancel (AccelTask.cancel(),
                               src/accel/tasks/mod.rs:88-95) */

#define LK_SOLVER_CHOLESKY 0 /* exact SPD solve: the reference's method (LAPACK sposv) */
#define LK_SOLVER_CG 1       /* tolerance-terminated conjugate gradient */
#define LK_SOLVER_AUTO 2     /* = Cholesky: exact at every k <= 256, like the reference */

const char *lk_last_error(void);
const char *lk_version(void);
/* Number of visible HIP devices (0 when there is no GPU / no driver). */
int lk_device_count(void);

/* Padded embedding width used on the device for `k` features: the next of
 * {16, 32, 64, 128, 256}; for 256 < k <= 1024 the next multiple of 64 (those sizes are solved on
 * tiles kept in HBM, csrc/als_big.hip: the reference's `POSV::solve`,
 * src/accel/als/solve.rs:65-107, takes any k); 0 if k is unsupported (k < 1 or k > 1024). */
int32_t lk_padded_dim(int32_t k);

/* Copy an [n x k] row-major matrix (leading dimension ld_src) into an
 * [n x ld_dst] one, zero-filling columns [k, ld_dst); and the inverse. */
int lk_pad_rows(const float *d_src, int64_t n, int32_t k, int32_t ld_src, float *d_dst,
                int32_t ld_dst, void *stream);
int lk_unpad_rows(const float *d_src, int64_t n, int32_t k, int32_t ld_src, float *d_dst,
                  int32_t ld_dst, void *stream);

/* ------------------------------------------------------------------------
 * Task control: cooperative cancel + live progress for the long-running entry points.
 * Replaces the `AccelTask` pyclass protocol (src/accel/tasks/mod.rs:33-106: `cancel()` sets a
 * flag the rayon workers poll, `current_progress()` reads an atomic row counter) that
 * `run_accel_task` drives from the main thread while `invoke` runs on a helper thread
 * (src/lenskit/parallel/_task.py:34-57).
 *   - the control block owns two words in pinned, device-mapped host memory: `cancel`
 *     (lk_task_ctl_cancel stores 1; callable from any thread while kernels run) and
 *     `rows_done` (the kernels post their running count there every 256 units;
 *     lk_task_ctl_progress reads it without touching the device or the stream);
 *   - attach it with lk_als_plan_set_ctl / lk_iknn_plan_set_ctl (NULL detaches); attached
 *     kernels skip every row (task) that has not started once the cancel is seen, and the
 *     entry point that synchronises next -- lk_als_check_status, lk_iknn_build_count,
 *     lk_iknn_build_fill -- returns LK_E_CANCELLED (outputs are then unspecified, like a
 *     cancelled rayon job's);
 *   - progress unit = rows (tasks/mod.rs:97-105); exact after the synchronising call.
 * Without a control block the kernels carry no polling code at all.
 * ---------------------------------------------------------------------- */
typedef struct lk_task_ctl lk_task_ctl;
int lk_task_ctl_create(lk_task_ctl **out);
void lk_task_ctl_destroy(lk_task_ctl *ctl);
void lk_task_ctl_cancel(lk_task_ctl *ctl);
int lk_task_ctl_cancelled(const lk_task_ctl *ctl);
/* clear the cancel flag and the progress count (before reusing the block) */
void lk_task_ctl_reset(lk_task_ctl *ctl);
int lk_task_ctl_progress(const lk_task_ctl *ctl, int64_t *rows_done, int64_t *rows_total);

/* ------------------------------------------------------------------------
 * Gramian:  out = M^T M + reg * I          (k x k, row-major, ld_out floats)
 * Replaces `_implicit_otor` (src/lenskit/als/_implicit.py:177-184), a NumPy
 * sgemm in the reference.  `d_ws` must hold lk_gramian_workspace_bytes(k).
 * Deterministic (fixed reduction order); the result is exactly symmetric.
 * ---------------------------------------------------------------------- */
size_t lk_gramian_workspace_bytes(int32_t k);
int lk_gramian(const float *d_m, int64_t n, int32_t k, int32_t ld, float reg, float *d_out,
               int32_t ld_out, void *d_ws, void *stream);

/* ------------------------------------------------------------------------
 * Implicit-feedback ALS half-epoch.
 * Replaces `lenskit._accel.als.train_implicit_matrix(matrix, this, other, otor)`
 * (src/lenskit/_accel/als.pyi:11-16; src/accel/als/implicit.rs:35-125 with
 * src/accel/als/solve.rs:65-107):  for every CSR row r
 *     A = otor + sum_j v_j q_j q_j^T,  y = sum_j (v_j + 1) q_j,  x = A^-1 y,
 *     this[r] <- x        (empty row: this[r] <- 0, contributes 0 to the delta)
 * and *d_out_frob = sqrt(sum_r ||x - this_old[r]||^2)  (float32, on device).
 *
 * A plan (row schedule: longest-first order, split of very long rows into
 * chunks, workspace layout) is built ONCE per matrix from the HOST copy of
 * indptr and reused for every epoch (csrc/als_plan.hip).  It also fixes which
 * kernel takes which rows: the ALS environment knobs of INTEGRATION.md are read
 * when the plan is created, not at every half-epoch.  It belongs to the device
 * current at creation; lk_als_plan_destroy may be called with any device current.
 * ---------------------------------------------------------------------- */
typedef struct lk_als_plan lk_als_plan;

/* Default plan = LK_ALS_PLAN_HYBRID_ORDER (round 5), unless the environment says
 * LK_ALS_RHS_ORDER=accurate (flags 0) or =reference (LK_ALS_PLAN_REFERENCE_ORDER). */
int lk_als_plan_create(lk_als_plan **out, const void *h_indptr, int indptr_is_64, int64_t n_rows,
                       int32_t k, int32_t solver);
/* The same with explicit flags (0 = the tuned kernels' own "accurate" summation everywhere).
 *
 * The reference's ARITHMETIC ORDER on long rows: `mtl.dot(&o_picked)`
 * (src/accel/als/implicit.rs:112) is matrixmultiply's sgemm, which sums the row's entries in
 * blocks of KC = 256 -- one fma chain per block, the block sums added one after the other -- and
 * `mt.dot(&vals)` (implicit.rs:117) is ONE sequential float32 chain per feature.  On rows of
 * 10^4 .. 10^6 entries those two sums drift systematically (1e-4 .. 7e-2 from the float64 sums),
 * so a kernel that sums more accurately lands that far from the REFERENCE's factors.
 *
 * LK_ALS_PLAN_HYBRID_ORDER (default): rows with more than LK_ALS_REF_LEN entries (environment,
 * default 2048 -- the rows that are pre-reduced in chunks anyway) are evaluated in the reference's
 * order: 256-entry chunks (one MFMA fmaf chain each, from zero), the chunk slabs added one after
 * the other in chunk order, OtOr last, y by the sequential chain of csrc/als_rhs.hip (bit-identical
 * to the reference's y).  Shorter rows keep the tuned order (the two agree to ~1e-5 there).  The
 * y buffer is part of the plan's workspace; works with task control, CSR views with row offsets
 * and any row / column relabelling (the chain runs over the row's entries as the CSR lists them:
 * give the rows in the reference's entry order -- ascending column of the ORIGINAL labelling).
 * k <= 256, exact solver; other plans ignore the flag.
 *
 * LK_ALS_PLAN_REFERENCE_ORDER: the strict variant -- EVERY row of more than 256 entries in
 * 256-entry chunks and every dense row's y by the chain; takes y from
 * lk_als_plan_set_rhs_workspace ([n_rows x lk_padded_dim(k)], mandatory for it), no task control.
 * tests/test_gpu_als_rhs_order.py.
 *
 * LK_ALS_PLAN_BAND_UNITS (with either of the above or alone): the caller will list the work units
 * band by band (lk_als_plan_order_units, below).  Hybrid plans at padded k = 64 then take a unit
 * per 256-entry block whatever their size -- the bands are tightest and the epoch measured fastest
 * that way; LK_ALS_REF_UNIT still overrides, and under LK_ALS_UNIT_ORDER=0 the
 * flag does nothing.  Other plans ignore it. */
#define LK_ALS_PLAN_REFERENCE_ORDER 1
#define LK_ALS_PLAN_HYBRID_ORDER 2
#define LK_ALS_PLAN_BAND_UNITS 4
int lk_als_plan_create_ex(lk_als_plan **out, const void *h_indptr, int indptr_is_64,
                          int64_t n_rows, int32_t k, int32_t solver, int32_t flags);
void lk_als_plan_destroy(lk_als_plan *plan);
/* Rows of the plan that are pre-reduced in chunks (longer than 2048 entries; LK_ALS_REF_LEN for
 * hybrid plans; 256 for strict reference-order plans): the first tasks of the longest-first
 * order, i.e. the rows sorted by descending length, ties in row order. */
int64_t lk_als_plan_long_rows(const lk_als_plan *plan);
/* The chunk kernel's work units of those rows: how many the plan has, and the CSR entries per
 * unit (a multiple of the 256-entry slab block).  Hybrid plans at padded k = 64 choose 1024, 512 or
 * 256 at creation -- the largest that leaves twice as many units as the device holds chunk waves
 * -- unless LK_ALS_REF_UNIT says otherwise. */
int64_t lk_als_plan_units(const lk_als_plan *plan);
int32_t lk_als_plan_unit(const lk_als_plan *plan);
/* Opt-in, once per plan at set-up, padded k <= 64: list the work units band by band instead of row
 * by row, so that the chunk workgroups resident on one XCD gather the same band of `other` at the
 * same time and share it in that XCD's L2.  A unit's key is the band it starts
 * in: col_key[c] of its first column c (`d_col_key`, n_col_key int32 words), or c itself when
 * d_col_key is NULL -- pass the map under which the rows' entries ascend (a relabelled engine
 * lists a row's entries by ascending ORIGINAL column: the map is original-of-new; first columns
 * outside the map keep c).  The units are sorted by (key, row, offset) and dealt so that the
 * workgroups one XCD receives (physical workgroup b on XCD b % 8) hold one contiguous run of the
 * sorted list, ascending along b; only the physically last workgroup may hold fewer than four
 * units.  Only the unit table moves: slabs, slab groups, the row order and every sum are what they
 * were, so no result changes by a bit.  Plans without long rows, plans of padded k > 64 and every
 * plan under LK_ALS_UNIT_ORDER=0 are left as they are; calling it again gives the same table.
 * Blocking (it waits for the device, copies the keys to the host and the table back): not for
 * plans built per call.  `d_indices` is the array the half-epochs are given. */
int lk_als_plan_order_units(lk_als_plan *plan, const int32_t *d_indices, const int32_t *d_col_key,
                            int64_t n_col_key, void *stream);
/* The unit table in launch order -- first CSR entry, entries and first slab of each of the
 * lk_als_plan_units units (any pointer may be NULL) -- by a blocking copy: tests and tools. */
int lk_als_plan_unit_table(const lk_als_plan *plan, int64_t *out_beg, int32_t *out_len,
                           int32_t *out_slab);
/* Hybrid plans: the right-hand sides of those rows as the last half-epoch run with workspace
 * `d_ws` formed them in the reference's order -- [lk_als_plan_long_rows x lk_padded_dim(k)]
 * floats, row t = the t-th longest row (device pointer into d_ws; NULL for other plans).
 * Diagnostic / test access: tests/test_gpu_als_rhs_order.py holds it to the chain bit for bit. */
const float *lk_als_plan_yref(const lk_als_plan *plan, const void *d_ws);
/* Device workspace the half-epoch needs (bytes); allocate once, reuse. */
size_t lk_als_plan_workspace_bytes(const lk_als_plan *plan);
/* Effective solver of the plan (LK_SOLVER_CHOLESKY or LK_SOLVER_CG). */
int32_t lk_als_plan_solver(const lk_als_plan *plan);

/* CG controls (ignored by the Cholesky solver): stop when ||r|| <= tol*||y|| or
 * after max_iter iterations (<=0: k iterations).  Defaults 1e-7 / k. */
int lk_als_plan_set_cg(lk_als_plan *plan, float tol, int32_t max_iter);
/* CG iterations spent and non-empty rows solved by the LAST CG half-epoch run with workspace
 * d_ws (sum over rows; blocking).  Diagnostic: the roofline of the CG kernel is
 * iterations * (4k flops per entry of the row + 2k^2). */
int lk_als_plan_cg_stats(const lk_als_plan *plan, void *d_ws, void *stream,
                         int64_t *out_iterations, int64_t *out_rows);
/* Attach a task-control block (cancel / progress) to every half-epoch run with this plan. */
int lk_als_plan_set_ctl(lk_als_plan *plan, lk_task_ctl *ctl);
/* Short rows at large k (implicit model, padded k = 128 / 256).  A row with n <= 64 entries
 * is a rank-n update of OtOr, the same matrix for every row of the half-epoch: with
 * Z = other * OtOr^-1 ([n_cols x lk_padded_dim(k)], pad columns zero) supplied by the caller,
 * lk_als_implicit_half_epoch solves those rows through the Woodbury identity (an n x n
 * system, O(n^2 k) instead of the k^3/3 of `sposv`, src/accel/als/solve.rs:65-107) -- the
 * same solution in exact arithmetic, no iteration (n <= 4 / 8: four / two rows per wave in one
 * 16 x 16 tile; n <= 16: one 16 x 16 system per wave; 17 .. 64: a 32 x 32 or 64 x 64 system on the
 * k <= 64 solver; 65 .. 128 at padded k = 256: a 128 x 128 system on the k = 128 blocked solver).  lk_als_plan_short_rows: how many rows of
 * the plan have <= 16 entries.  lk_als_plan_set_z: Z for the NEXT half-epoch calls (NULL: every row
 * takes the dense solve); the buffer must stay alive until those calls have finished. */
int64_t lk_als_plan_short_rows(const lk_als_plan *plan);
/* rows the 16 x 16 ... 64 x 64 Woodbury systems take: <= 64 entries at padded k = 256 (rows of
 * 65 .. 128 entries additionally take a 128 x 128 system there unless LK_ALS_WB128=0); at padded
 * k = 128 <= 64 / 32 / 16 entries with LK_ALS_WB64_K128 = 64 (default) / 32 / 0 at plan creation */
int64_t lk_als_plan_woodbury_rows(const lk_als_plan *plan);
int lk_als_plan_set_z(lk_als_plan *plan, const float *d_z);
/* The same path with NOTHING computed on the caller's side: hand the plan a device buffer of
 * n_cols x lk_padded_dim(k) floats and every lk_als_implicit_half_epoch run with it forms Z
 * itself on the launch stream -- OtOr^-1 to float64 accuracy by an in-register sweep + two
 * Newton-Schulz steps (csrc/spd_inverse.hip), then Z = other * OtOr^-1 on the scoring GEMM.  If
 * OtOr turns out not to be positive definite (reg = 0 with rank-deficient factors) the decision
 * is taken ON THE DEVICE: the Woodbury kernels stand down and a dense fallback launch solves
 * their rows exactly as `sposv` would (and reports a row whose own matrix is not positive
 * definite the same way).  No library call, no host synchronisation.  NULL detaches the buffer. */
int lk_als_plan_set_z_workspace(lk_als_plan *plan, float *d_zbuf);
/* Strict reproduction of the reference's right-hand side.  `train_row_solve` forms
 * y = mt.dot(&vals) on a TRANSPOSED (strided) view (src/accel/als/implicit.rs:116-117;
 * explicit model: src/accel/als/explicit.rs:110), which ndarray evaluates as ONE sequential
 * float32 chain per feature over the row's entries, product and sum rounded separately.  On rows
 * of 10^5 .. 10^6 entries that chain drifts 1e-4 .. 7e-2 from the exact sum; the solve kernels'
 * own (slotted / chunked) sum does not, so on such rows the default result is CLOSER TO FLOAT64
 * THAN THE REFERENCE IS and can be > 1e-4 away from it.  Hand the plan a device buffer of
 * n_rows x lk_padded_dim(k) floats and every half-epoch (implicit and explicit) first forms y in
 * exactly the reference's order (csrc/als_rhs.hip: lane = feature, entries in row order) and the
 * dense solve kernels take their right-hand side from it -- bit-identical y, so those rows land
 * within 1e-4 of the reference.  Slower (one latency-bound chain per feature); rows served by
 * the Woodbury kernels (<= 64 entries at padded k > 64) never form y and are unaffected; ignored
 * while a task-control block is attached.  NULL detaches (default: the accurate sum). */
int lk_als_plan_set_rhs_workspace(lk_als_plan *plan, float *d_y);
/* Several plans over ROW SLICES of one half-epoch (the sharded engine cuts a rank's rows into
 * slices so that the all-gather of one slice runs under the solve of the next) share one Z: the
 * leading slice's plan owns the buffer (lk_als_plan_set_z_workspace) and is launched first; the
 * others are given that buffer and the device address of the leader's "OtOr is not positive
 * definite" flag (lk_als_plan_z_flag(leader, leader's workspace)), which they copy into their
 * own status word at every launch -- same stream, so it is final by then.  NULL / NULL detaches. */
int lk_als_plan_set_z_shared(lk_als_plan *plan, const float *d_z, const void *d_flag);
int lk_als_plan_set_z_leader(lk_als_plan *plan, int on); /* form Z even without short rows of its own */
const void *lk_als_plan_z_flag(const lk_als_plan *plan, const void *d_ws);
/* OtOr^-1 alone (diagnostics / tests): d_out [KP x KP] floats zero padded, *d_flag = 0 or != 0
 * when d_a is not positive definite, d_ws lk_spd_inverse_workspace_bytes(k) bytes; padded
 * k = 128 / 256 only. */
size_t lk_spd_inverse_workspace_bytes(int32_t k);
int lk_spd_inverse(const float *d_a, int32_t lda, int32_t k, float *d_out, int32_t *d_flag,
                   void *d_ws, void *stream);

int lk_als_implicit_half_epoch(const lk_als_plan *plan, const void *d_indptr,
                               const int32_t *d_indices, const float *d_values, int64_t n_rows,
                               int64_t n_cols, int32_t k, float *d_this, int32_t ld_this,
                               const float *d_other, int32_t ld_other, const float *d_otor,
                               int32_t ld_otor, void *d_ws, float *d_out_frob, void *stream);
/* One whole implicit epoch -- user half, P^T P + item_reg I, item half, Q^T Q + user_reg I -- in one
 * call, with the two halves' small kernels scheduled off the critical path:
 * the Gramian of the new P and the item half's primed copy of it run on the user plan's side
 * stream under the item half's chunk kernel, and the long rows of each half are solved on that
 * half's side stream right behind their slab sums.  Results are bit for bit those of
 *   lk_als_implicit_half_epoch(user) ; lk_gramian(P) ; lk_als_implicit_half_epoch(item) ; lk_gramian(Q).
 * Serves what the flagship runs and nothing else: two DIFFERENT plans with the same k, padded
 * k <= 64, the exact solver, LK_ALS_PLAN_HYBRID_ORDER, no task-control block, one device
 * (LK_E_INVALID otherwise: use the calls above).  P [user rows x lk_padded_dim(k)] and Q are
 * updated in place; d_qtq holds Q^T Q + user_reg I (ld_qtq >= k) on entry and the new one on
 * return, d_ptp receives P^T P + item_reg I; d_gram_ws is lk_gramian_workspace_bytes(k) bytes;
 * d_out_delta[0] = |dP|, d_out_delta[1] = |dQ| (written directly: no copy).  Both status words
 * are read with lk_als_check_status as before.  When the call returns, everything it enqueued --
 * on the plans' side streams too -- is ordered before whatever `stream` receives next.
 * (The half-epoch calls at padded k <= 64 share the launch code: without a task-control block
 * their long-row solve launch -- hybrid and strict reference-order plans, implicit and explicit
 * model -- now also runs on the plan's side stream behind the slab sums, joined before the
 * delta reduction.  Same kernels, same results, same ordering guarantee on `stream`.) */
int lk_als_implicit_epoch(const lk_als_plan *user_plan, const lk_als_plan *item_plan,
                          const void *d_u_indptr, const int32_t *d_u_indices,
                          const float *d_u_values, const void *d_i_indptr,
                          const int32_t *d_i_indices, const float *d_i_values, int32_t k,
                          float *d_p, float *d_q, float *d_qtq, int32_t ld_qtq, float user_reg,
                          float *d_ptp, int32_t ld_ptp, float item_reg, void *d_user_ws,
                          void *d_item_ws, void *d_gram_ws, float *d_out_delta, void *stream);
/* Explicit-feedback (biased-MF) half-epoch: replaces `_accel.als.train_explicit_matrix(matrix,
 * this, other, reg)` (src/lenskit/_accel/als.pyi, src/accel/als/explicit.rs:33-119):
 *   A = sum_j q_j q_j^T + reg * n * I,  A x = sum_j r_j q_j   (r = bias-normalised ratings),
 * empty rows -> zeros; same plan, workspace, in-place update, status word and return value
 * (sqrt of the summed squared row deltas at d_out_frob) as the implicit form.  Exact solver
 * only. */
int lk_als_explicit_half_epoch(const lk_als_plan *plan, const void *d_indptr,
                               const int32_t *d_indices, const float *d_values, int64_t n_rows,
                               int64_t n_cols, int32_t k, float *d_this, int32_t ld_this,
                               const float *d_other, int32_t ld_other, float reg, void *d_ws,
                               float *d_out_frob, void *stream);
/* Optional per-kernel timing with HIP events recorded on the launch stream
 * (bench.py's roofline leg).  get_timing waits for the recorded events, returns the
 * summed durations (ms) of the chunk kernel and of the solve kernel over the
 * *n_launches half-epochs recorded since the last call (at most 128), and resets. */
int lk_als_plan_enable_timing(lk_als_plan *plan, int enable);
int lk_als_plan_get_timing(lk_als_plan *plan, double *ms_chunk, double *ms_solve,
                           int32_t *n_launches);

/* Synchronise `stream` and translate the device status word of the last
 * half-epoch into a return code (LK_E_NOT_SPD with the offending row in
 * lk_last_error()).  Call before trusting `this`. */
int lk_als_check_status(const lk_als_plan *plan, void *d_ws, void *stream);

/* Host-pointer convenience form with the reference's exact argument list
 * (`train_implicit_matrix(matrix, this, other, otor)`, src/accel/als/implicit.rs:35-84:
 * this: [n_rows x k] updated in place, other: [n_cols x k], otor: [k x k], all C-contiguous
 * host float32; offsets int32 or int64).  Allocates, copies, runs (default plan: hybrid
 * summation order; padded k = 128 / 256: the Woodbury kernels for the short rows when there
 * are >= LK_ALS_WB_MIN_ROWS of them), copies back; blocking.  Errors: LK_E_NOT_SPD with
 * "ALS solve error: ..." in lk_last_error() (implicit.rs:79), `this` left untouched.
 * tests/test_gpu_host_abi.py runs INTEGRATION.md's binding sketch through it with raw ctypes. */
int lk_als_implicit_half_epoch_host(const void *h_indptr, int indptr_is_64,
                                    const int32_t *h_indices, const float *h_values,
                                    int64_t n_rows, int64_t n_cols, int32_t k, float *h_this,
                                    const float *h_other, const float *h_otor, int32_t solver,
                                    float *h_out_frob);
/* The same with the reference's task controls (src/accel/tasks/mod.rs:62-106,
 * src/lenskit/parallel/_task.py:25-57): `ctl` (may be NULL) is polled by the running kernels --
 * lk_task_ctl_cancel from another thread makes the call return LK_E_CANCELLED with the rows
 * solved so far written to `this` (the reference updates `this` in place row by row as well);
 * lk_task_ctl_progress reads the live count of finished rows.  With a control block every row
 * takes the dense kernels (the Woodbury kernels do not poll). */
int lk_als_implicit_half_epoch_host_ctl(const void *h_indptr, int indptr_is_64,
                                        const int32_t *h_indices, const float *h_values,
                                        int64_t n_rows, int64_t n_cols, int32_t k, float *h_this,
                                        const float *h_other, const float *h_otor,
                                        int32_t solver, float *h_out_frob, lk_task_ctl *ctl);

/* ------------------------------------------------------------------------
 * Item-item similarity build.
 * Replaces `lenskit._accel.knn.compute_similarities(ui, iu, shape, min_sim,
 * save_nbrs)` (src/lenskit/_accel/knn.pyi:8-14; src/accel/knn/item_train.rs:33-152
 * + src/accel/sparse/consumer.rs:24-142): for each item i,
 *     dots[j] = sum over users u of i (ascending u) of a_ui * a_uj   (j != i)
 * accumulated in f32 as round(a_ui*a_uj) then add -- the reference's order and
 * rounding, so values are bit-identical -- keep dots[j] >= min_sim, optional
 * per-row top-`save_nbrs` (by similarity, ties by first encounter), rows sorted
 * by column.  Output CSR has int64 offsets (LargeList).
 *
 * Two-phase because the output size is data dependent:
 *   lk_iknn_build_count  -> fills d_out_indptr (n_items+1, int64, exclusive scan)
 *                           and returns the total through *h_total_nnz (blocking);
 *   lk_iknn_build_fill   -> writes d_out_indices / d_out_values.
 * Both calls take the SAME workspace (it carries the per-task counts / offsets
 * between them).  When n_items^2 (index, value) pairs fit comfortably in free HBM
 * (cap: env LK_IKNN_STAGE_GB, default 64) the plan reserves a staging area in the
 * workspace: the count call then does the whole computation once and the fill call
 * only compacts; otherwise each call is a full pass over the data.
 * ---------------------------------------------------------------------- */
typedef struct lk_iknn_plan lk_iknn_plan;
int lk_iknn_plan_create(lk_iknn_plan **out, const void *h_ui_indptr, const void *h_iu_indptr,
                        int indptr_is_64, int64_t n_users, int64_t n_items);
/* Shard of the build: output rows (items) [row_begin, row_end) only -- rows are independent
 * (`compute_similarities` is a par_iter over rows, item_train.rs:56-70), so ranks of a
 * multi-GPU job each build a row block with no collective.  d_out_indptr then has
 * (row_end - row_begin + 1) entries; column numbers stay global. */
int lk_iknn_plan_create_rows(lk_iknn_plan **out, const void *h_ui_indptr,
                             const void *h_iu_indptr, int indptr_is_64, int64_t n_users,
                             int64_t n_items, int64_t row_begin, int64_t row_end);
void lk_iknn_plan_destroy(lk_iknn_plan *plan);
int lk_iknn_plan_set_ctl(lk_iknn_plan *plan, lk_task_ctl *ctl);
/* Optional timing of the similarity kernel with HIP events recorded on the launch stream
 * (bench.py's roofline leg): get_timing waits for the events, returns the summed duration
 * (ms) of the build-kernel launches recorded since the last call (one for a staged build,
 * two for a two-pass build) and resets. */
int lk_iknn_plan_enable_timing(lk_iknn_plan *plan, int enable);
int lk_iknn_plan_get_timing(lk_iknn_plan *plan, double *ms_build, int32_t *n_launches);
size_t lk_iknn_plan_workspace_bytes(const lk_iknn_plan *plan);

int lk_iknn_build_count(const lk_iknn_plan *plan, const void *d_ui_indptr,
                        const int32_t *d_ui_indices, const float *d_ui_values,
                        const void *d_iu_indptr, const int32_t *d_iu_indices,
                        const float *d_iu_values, float min_sim, int64_t save_nbrs, void *d_ws,
                        int64_t *d_out_indptr, int64_t *h_total_nnz, void *stream);
int lk_iknn_build_fill(const lk_iknn_plan *plan, const void *d_ui_indptr,
                       const int32_t *d_ui_indices, const float *d_ui_values,
                       const void *d_iu_indptr, const int32_t *d_iu_indices,
                       const float *d_iu_values, float min_sim, int64_t save_nbrs, void *d_ws,
                       const int64_t *d_out_indptr, int32_t *d_out_indices, float *d_out_values,
                       void *stream);

/* ------------------------------------------------------------------------
 * Dense scoring with fused top-K.
 * Replaces, for a batch of users, `ALSBase.__call__` scoring
 * (src/lenskit/als/_common.py:159-170: scores = Q u) followed by
 * `TopNRanker` -> `ItemList.top_n` -> `_accel.data.argtopn`
 * (src/lenskit/basic/topn.py:45-69, src/lenskit/data/_items.py:942-998,
 * src/accel/data/sorting.rs:132-172).
 *   scores[b][i] = fma-chain over f = 0..k-1 of U[b][f]*Q[i][f]  (f32 MFMA: exact,
 *   k-ordered) for every item i not listed in the exclusion CSR row b
 *   (candidate selector: training items minus the query's items,
 *   src/lenskit/basic/candidates.py:77-94); NaN scores are skipped;
 *   out_idx[b][0..n) = indices of the n largest scores, descending, ties by
 *   lower index; out_score likewise; rows with fewer than n candidates are
 *   padded with index -1 / score NaN.
 * Two implementations, identical results bit for bit:
 *   - fused (n <= 128, >= 16384 items, >= 8192 users, k > 16; env LK_TOPK_FUSED_MIN_ITEMS /
 *     LK_TOPK_FUSED_MIN_USERS): a threshold per user from an item sample, then ONE pass of
 *     the contraction whose epilogue keeps only the entries that reach it, then the exact order
 *     among those candidates -- the n_users x n_items score matrix never exists in memory;
 *     this path synchronises the stream before returning (it reads the list of rows that did
 *     not end up with n valid candidates -- overflowing lists, thresholds that proved too
 *     high -- and redoes exactly those rows through the panel path);
 *   - panel: 2048 users at a time are scored into the workspace and selected from there.
 * Workspace (ask lk_score_topk_workspace_bytes, never assume): the fused path works on batches
 * of up to 262 144 users (LK_TOPK_FUSED_ROWS; 65 536 before round 3) and holds per batch
 * 16 KiB of candidate lists per user (<= 4 GiB) plus the stage-1 sample panel,
 * users x ceil(n_items / 16) floats, which is what bounds the batch: never more than 16 GiB
 * (for catalogues so large that 8192 sample rows would exceed it the batch shrinks below 8192
 * rather than the panel growing).  Ceiling: ~20.5 GiB, reached only with >= 262 144 users and
 * >= 250 000 items; ML-25M (162 541 x 62 423): 5.3 GiB.  The panel path needs 2048 x n_items
 * floats.
 * ---------------------------------------------------------------------- */
size_t lk_score_topk_workspace_bytes(int64_t n_users, int64_t n_items, int32_t n);
int lk_score_topk(const float *d_users, int32_t ld_users, int64_t n_users, const float *d_items,
                  int32_t ld_items, int64_t n_items, int32_t k, int32_t n,
                  const int64_t *d_excl_ptr, const int32_t *d_excl_items, void *d_ws,
                  int32_t *d_out_idx, float *d_out_score, void *stream);
/* Test hook: what the calling thread's last lk_score_topk call did, from values the host holds
 * anyway (no launch, copy or synchronisation of its own).  out12 = {path: 1 fused, 0 panel, -1 no
 * call yet; fused batches; parts of the item split (1: none); candidates per part; 1 if a batch
 * ran its two row ranges on two streams; rows listed for the exact redo; 1 if that list
 * overflowed and EVERY row went through the panel path; sample stride; sample items; threshold
 * rank of a row without exclusions; padded features; 1 class-maxima / 0 sample-panel stage 1}
 * (everything after `path` is 0 for a panel call, the padded features excepted).  The rows redone
 * one by one (at most 4096, in the order the device listed them) are copied to redo_rows[0 .. cap);
 * returns how many were copied.  Product code must not read it. */
int32_t lk_score_topk_last_report(int64_t *out12, int32_t *redo_rows, int32_t cap);

/* Scores only: out[b][i] = the same exact k-ordered chain, for every (user, item) pair
 * (`ALSBase.__call__`, src/lenskit/als/_common.py:159-170). */
int lk_score_dense(const float *d_users, int32_t ld_users, int64_t n_users, const float *d_items,
                   int32_t ld_items, int64_t n_items, int32_t k, float *d_out, int64_t ld_out,
                   void *stream);

/* Plain top-N over score vectors already in HBM (one row per query), the direct stand-in for
 * `_accel.data.argtopn(scores, n)` (src/accel/data/sorting.rs:132-172) and, with n < 0, for
 * `_accel.data.argsort_descending(scores)` (sorting.rs:69-103): every valid entry by descending
 * score.  d_out_idx is [n_rows x min(n, row_len)] (n < 0: [n_rows x row_len]), -1 padded.
 * n <= 4096 runs the selection kernel and needs no workspace; n < 0 or n > 4096 is a full
 * stable sort and needs lk_argtopn_workspace_bytes(n_rows, row_len, n) bytes at d_ws.
 * (lk_score_topk likewise: n < 0 ranks all candidates, output [n_users x n_items].) */
size_t lk_argtopn_workspace_bytes(int64_t n_rows, int64_t row_len, int32_t n);
int lk_argtopn(const float *d_scores, int64_t n_rows, int64_t row_len, int32_t n, void *d_ws,
               int32_t *d_out_idx, void *stream);

/* Per-row top-`save_nbrs` truncation of a built similarity matrix -- the second half of
 * `sim_row` (src/accel/knn/item_train.rs:139-151): keep the save_nbrs most similar
 * neighbours of every row, ties at the cut in order of first encounter (first shared user,
 * then column), rows stay sorted by column.  lk_iknn_build_* take save_nbrs <= 0 (none);
 * run these on their output.  `nnz` = entries of the input matrix.  _count is blocking. */
size_t lk_iknn_truncate_workspace_bytes(int64_t n_rows, int64_t nnz);
/* n_rows rows of the similarity matrix; row r is item (row_begin + r) (0 for a full build) */
int lk_iknn_truncate_count(const int64_t *d_sim_indptr, const int32_t *d_sim_indices,
                           const float *d_sim_values, const void *d_iu_indptr,
                           int iu_indptr_is_64, const int32_t *d_iu_indices, int64_t n_rows,
                           int64_t row_begin, int64_t nnz, int64_t save_nbrs, void *d_ws,
                           int64_t *d_out_indptr, int64_t *h_total_nnz, void *stream);
int lk_iknn_truncate_fill(const int64_t *d_sim_indptr, const int32_t *d_sim_indices,
                          const float *d_sim_values, int64_t n_rows, int64_t nnz, void *d_ws,
                          const int64_t *d_out_indptr, int32_t *d_out_indices,
                          float *d_out_values, void *stream);

/* ------------------------------------------------------------------------
 * Item-kNN "recommend" for a BATCH of queries: score EVERY item and keep the top n.
 * Replaces, for a batch, what `pipelines/iknn-explicit.toml`'s recommender runs per query
 * (src/lenskit/batch/_runner.py:283-308): the candidate selector (all training items minus the
 * query's own, src/lenskit/basic/candidates.py:77-94), `ItemKNNScorer.__call__` over the
 * candidates (src/lenskit/knn/item.py:231-295 -> `score_explicit` / `score_implicit`,
 * src/accel/knn/item_score.rs:23-111, accum.rs), the item means added back (item.py:282), and
 * `TopNRanker` (src/lenskit/basic/topn.py:45-69 -> src/accel/data/sorting.rs:132-172).
 *   query q: reference items ref_items[ref_ptr[q]..ref_ptr[q+1]) (negative = null, skipped) with
 *   centred ratings ref_rates (NULL => implicit feedback); d_item_bias NULL or [n_items] floats
 *   added to every score (one f32 add, as NumPy's `scores + means`); exclude_refs != 0 strikes
 *   the query's own items from the candidates; items with fewer than min_nbrs contributors have
 *   no score and are never listed.  out_idx [n_queries x n] = the n best scored items,
 *   descending, ties by lower item number, -1 padded; out_score likewise (NaN padded; may be
 *   NULL).  n < 0: every scored candidate, ranked (output [n_queries x n_items]).
 *   The SCORES are the reference accumulator's bit for bit (csrc/iknn_recommend.hip: one wave
 *   per (query, window of 4096 items); round 6: every weight is added to its item's LDS cell by
 *   ds_add_f32 in history order -- the LDS applies same-address adds in lane order, probed on the
 *   device --, items with more than max_nbrs contributors are found again and replayed on the
 *   reference's heap by a kernel of their own; the list kernel of rounds 4-5 -- hits laid out per
 *   item through in-order LDS cursors -- is the fallback.  No barrier per history row as in
 *   lk_iknn_score_batch's slot kernel).
 *   h_query_hits (HOST, [n_queries]): per query, the summed lengths of its reference items'
 *   similarity rows (the caller has the row lengths: `item_counts`); max_query_hits >= their
 *   maximum sizes the workspace (the list kernel's hit region, the queue of heap items: at most
 *   hits / (max_nbrs + 1) per query).  Queries are processed in batches of <= 6144
 *   (LK_REC_PANEL_ROWS), <= 2^28 hits and a full queue at most; a call of several batches keeps
 *   two score panels (LK_REC_PANEL_GB bounds them) and runs a batch's selection on a side stream
 *   while the next batch is scored.  Blocking (returns LK_E_NAN_SIM for a NaN similarity).
 * ---------------------------------------------------------------------- */
size_t lk_iknn_recommend_workspace_bytes(int64_t n_items, int64_t n_queries,
                                         int64_t max_query_hits, int32_t max_nbrs, int32_t n);
int lk_iknn_recommend(const int64_t *d_sim_indptr, const int32_t *d_sim_indices,
                      const float *d_sim_values, int64_t n_items, int64_t n_queries,
                      const int64_t *d_ref_ptr, const int32_t *d_ref_items,
                      const float *d_ref_rates, const float *d_item_bias, int32_t max_nbrs,
                      int32_t min_nbrs, int32_t n, int exclude_refs, const int64_t *h_query_hits,
                      int64_t max_query_hits, void *d_ws, int32_t *d_out_idx, float *d_out_score,
                      void *stream);

/* ------------------------------------------------------------------------
 * Item-kNN scoring for a BATCH of queries.
 * Replaces `_accel.knn.score_explicit` / `score_implicit`
 * (src/lenskit/_accel/knn.pyi:15-29; src/accel/knn/item_score.rs:23-111,
 * src/accel/knn/accum.rs:16-239), which score ONE query per call.
 *   query q has reference (history) items ref_items[ref_ptr[q]..ref_ptr[q+1]) with
 *   centred ratings ref_rates (NULL => implicit) and targets
 *   tgt_items[tgt_ptr[q]..tgt_ptr[q+1]); negative item numbers are nulls.
 *   score_t = sum_{top max_nbrs by sim} s*v / sum s  (explicit)  or  sum s (implicit);
 *   fewer than min_nbrs contributors => NaN.  out_counts = contributors kept
 *   (-1 for a null target).  Blocking (returns LK_E_NAN_SIM for a NaN similarity).
 *   Calls in which no query has more than 1024 targets, with max_nbrs <= 255, take the
 *   candidate-list kernel: targets hashed in LDS, all history rows streamed at once, and the
 *   reference's accumulator followed step for step (a vector, then std's BinaryHeap push / pop),
 *   so that WHICH of several equal similarities is evicted at the max_nbrs boundary and the order
 *   of the f32 sums are the reference's: the scores are bit-identical to its.  Other calls
 *   (`score every item`) take the one-history-row-at-a-time slot kernel, which runs the same
 *   accumulator on per-item slots of the workspace (bit-identical as well, slower per target).
 *   LK_KNN_SCORE_LISTS=0 forces the slot kernel.  The matrix rows must not name a column twice
 *   (LK_E_INVALID from the list kernel).  lk_knn_score_last_stats: of the calling thread's last
 *   call, {queries scored by the list kernel, by the slot kernel, longest target list} (test hook).
 * ---------------------------------------------------------------------- */
size_t lk_iknn_score_workspace_bytes(int64_t n_items, int64_t n_queries, int32_t max_nbrs);
void lk_knn_score_last_stats(int64_t *out3);
/* 2 / 1 / 0: the last lk_iknn_recommend call of this process ran the ACCUMULATING kernel (round 6,
 * the default: weights added to their target's LDS cell by ds_add_f32 -- same-address adds of an
 * instruction applied in lane order with the VALU's rounding, probed on the device at first use),
 * the list kernel walking the similarity rows PACKED (64 entries of several (row x window) pieces
 * per instruction; needs same-address LDS atomics of one instruction served in lane order, probed
 * as well; LK_REC_ACC=0 forces it), or the list kernel piece by piece (LK_REC_PACKED=0); -1: no
 * call yet.  Test hook.  Same scores in all three.  LK_REC_OVERLAP=0: the batches' tails (queued
 * targets, selection) on the caller's stream instead of a side stream. */
int lk_iknn_recommend_last_packed(void);
int lk_iknn_score_batch(const int64_t *d_sim_indptr, const int32_t *d_sim_indices,
                        const float *d_sim_values, int64_t n_items, int64_t n_queries,
                        const int64_t *d_ref_ptr, const int32_t *d_ref_items,
                        const float *d_ref_rates, const int64_t *d_tgt_ptr,
                        const int32_t *d_tgt_items, int32_t max_nbrs, int32_t min_nbrs,
                        void *d_ws, float *d_out_scores, int32_t *d_out_counts, void *stream);

/* ------------------------------------------------------------------------
 * The rating-predictor tail of std:topn-predict for a BATCH of queries (csrc/predict_merge.hip);
 * `batch.predict` calls it after lk_iknn_score_batch so that no score, count or flag goes back
 * to the host one query at a time.  Both calls are asynchronous on `stream`.
 *
 * lk_bias_user_offsets replaces, for a whole batch, the user bias that
 * `BiasModel.compute_for_items` takes from the query's training ratings
 * (src/lenskit/basic/bias.py:166-240): query q's history is row d_user_nums[q] of the training
 * matrix (offsets i32/i64, item numbers, ratings f32; -1 or out of range: no training row);
 *   uoff_j = (double)r_j - global_bias [- (double)d_item_biases[item_j]]  (d_item_biases NULL:
 *   no item term), ub = sum_j uoff_j / ((double)count of finite uoff_j + damping_user), a NaN
 *   ub becomes 0, rounded to float32 at the end.  The sum is NumPy's `np.sum` of a contiguous
 *   float64 array, its pairwise order included (blocks of 8192 in sequence, 8-accumulator leaves
 *   of <= 128 elements), so ub is the host's bit for bit.  d_out_ub [n_queries] = ub (0 without
 *   a row); d_out_add [n_queries] = 1 where the query has a training row (the host adds ub only
 *   then: -0.0 + 0.0 is +0.0), 0 elsewhere.  One wave per query.
 *
 * lk_predict_merge replaces the item-mean add-back of `ItemKNNScorer.__call__`
 * (src/lenskit/knn/item.py:282) and `FallbackScorer` (src/lenskit/basic/composite.py) over a
 * `BiasScorer`: for every entry e of query q (d_tgt_ptr [n_queries + 1] int64 offsets into
 * d_tgt_items / d_scores, n_entries = d_tgt_ptr[n_queries]; negative or >= n_items targets are
 * unknown items) in float32:  s = d_scores[e] (+ d_item_means[t] when not NULL and t is known);
 * with `fallback` != 0, a NaN s becomes (float)global_bias (+ d_item_biases[t] when not NULL
 * and t is known) (+ d_user_bias[q] where d_user_add[q] != 0; d_user_add NULL: never) and
 * d_out_is_fallback[e] = 1 (0 elsewhere; the flags may be NULL).  d_scores is updated in place.
 * ---------------------------------------------------------------------- */
int lk_bias_user_offsets(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                         const float *d_values, int64_t n_users, int64_t n_items,
                         int64_t n_queries, const int32_t *d_user_nums, double global_bias,
                         const float *d_item_biases, double damping_user, float *d_out_ub,
                         uint8_t *d_out_add, void *stream);
int lk_predict_merge(int64_t n_queries, const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                     int64_t n_entries, int64_t n_items, float *d_scores,
                     const float *d_item_means, int fallback, double global_bias,
                     const float *d_item_biases, const float *d_user_bias,
                     const uint8_t *d_user_add, uint8_t *d_out_is_fallback, void *stream);

/* ------------------------------------------------------------------------
 * The bias model on the device (csrc/bias.hip): the fit of `BiasModel.learn`
 * (src/lenskit/basic/bias.py:83-150) and `BiasScorer`'s score for whole batches.  All calls are
 * asynchronous on `stream`; there is no atomic in any of them.
 *
 * lk_bias_fit_pass is ONE pass of the fit over the bins of a CSR (offsets i32/i64; a bin is a
 *   row): the item pass over the transposed ratings (lk_csr_transpose is stable, so an item's
 *   entries are in dataset order), the user pass over the ratings themselves.  For bin b, in the
 *   order of its entries e,
 *     c[e]  = d_values[e] -f32 (float)global_bias  [-f32 d_sub[d_indices[e]]]   (d_sub NULL: no
 *             second term; d_indices is read only with d_sub, n_sub = its length)
 *     sum   = 0.0 + (double)c[e0] + (double)c[e1] + ...     one float64 chain, never reassociated
 *     count = damping + 1.0 + 1.0 + ...                      a chain too: NOT damping + n
 *     d_out[b] = (float)(sum / count) where count > 0, else 0
 *   which are the bits of the host's `np.add.at` / `np.divide(..., where=counts > 0)`.  A bin of at
 *   most lk_bias_fit_short_max() entries is summed by one lane, a longer one by one wave that
 *   loads lk_bias_fit_chunk() entries at a time.
 * lk_bias_score_panel writes d_panel [n_rows x n_items] (rows `ld` floats apart):
 *   cell (q, i) = ((float)global_bias +f32 d_item_biases[i]) +f32 d_user_bias[q], the item term
 *   only with d_item_biases, the user term only where d_user_add[q] != 0 (NULL: never) -- what
 *   lk_bias_user_offsets returns.  With d_user_nums (int32 [n_rows]; NULL: nothing is struck) the
 *   cells of row q at the items of row d_user_nums[q] of the training matrix (d_hist_indptr
 *   i32/i64, d_hist_indices; -1 or >= n_users: no row) are then set to NaN.
 * lk_bias_score_ragged writes the same cell for every entry e of query q (d_tgt_ptr int64
 *   [n_queries + 1] offsets into d_tgt_items, n_entries = d_tgt_ptr[n_queries]) to d_out[e]; a
 *   negative or >= n_items target is an unknown item, whose cell has no item term -- it is NOT
 *   NaN (`BiasModel.compute_for_items`, bias.py:166-241).
 * ---------------------------------------------------------------------- */
int32_t lk_bias_fit_short_max(void);
int32_t lk_bias_fit_chunk(void);
int lk_bias_fit_pass(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                     const float *d_values, int64_t n_bins, double global_bias,
                     const float *d_sub, int64_t n_sub, double damping, float *d_out,
                     void *stream);
int lk_bias_score_panel(int64_t n_rows, int64_t n_items, double global_bias,
                        const float *d_item_biases, const float *d_user_bias,
                        const uint8_t *d_user_add, float *d_panel, int64_t ld,
                        const void *d_hist_indptr, int indptr_is_64,
                        const int32_t *d_hist_indices, int64_t n_users,
                        const int32_t *d_user_nums, void *stream);
int lk_bias_score_ragged(int64_t n_queries, const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                         int64_t n_entries, int64_t n_items, double global_bias,
                         const float *d_item_biases, const float *d_user_bias,
                         const uint8_t *d_user_add, float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * `BiasedMFScorer.__call__` for a BATCH of queries (csrc/bmf_batch.hip): the host arithmetic of
 * the explicit-feedback ALS scorer around its row solve and its lk_score_dense row
 * (src/lenskit/als/_common.py:133-175, _explicit.py:55-91, basic/bias.py:166-241), so that a
 * batched list holds float32(the per-query score) bit for bit.  A query's MODE says which branch
 * the per-query path takes, and with it the precision it adds in:
 *   LK_BMF_FOLD    a fold-in row: ub is the float64 user bias derived from the history, and
 *                  score = (float)((double)dot + ((double)((float)mu + b_i) + ub));
 *   LK_BMF_STORED  the stored embedding: ub holds the model's float32 user bias (exactly), and
 *                  score = dot + (((float)mu + b_i) + (float)ub) in float32;
 *   LK_BMF_INVALID neither: the score is NaN.
 * `dot` is the lk_score_dense entry; d_item_biases [n_items] f32 is required.
 *
 * lk_bmf_residual_rows: query q's history is row d_user_nums[q] of the training matrix (as
 *   lk_bias_user_offsets takes it; -1 or out of range: no row, ub = 0, nothing written).
 *   d_out_ub[q] = the ub of lk_bias_user_offsets BEFORE its rounding to float32 (same sum, same
 *   order); the row's entries go to d_out_indices / d_out_values from d_out_ptr[q] on (int64
 *   [n_queries + 1], the caller's prefix sums of the row lengths; entries past d_out_ptr[q + 1]
 *   are not written), item numbers copied, values r_j - (((float)mu + b_i[j]) + (float)ub) in
 *   float32: the CSR `new_user_embedding` hands to the explicit row solve.  One wave per query.
 * lk_bmf_finish_panel: the finish in place on d_panel [n_rows x n_items], rows `ld` floats apart,
 *   16-byte aligned; d_mode uint8 [n_rows], d_ub float64 [n_rows].  With d_strike_ptr (int64
 *   [n_rows + 1] offsets into d_strike_items, int32) each row's listed items are then set to NaN.
 * lk_bmf_finish_pairs: entries first_entry .. first_entry + n_entries - 1 of the ragged lists
 *   d_tgt_ptr [n_rows + 1] / d_tgt_items (d_tgt_ptr[0] = first_entry; negative or >= n_items: an
 *   unknown item, NaN): d_out[e] = the finish of d_panel[row of e][d_tgt_items[e]].
 * lk_bmf_finish_ragged: the same finish where the dot products are ragged already: d_dots f32
 *   [total] holds the lk_score_dense entry of (row of e, d_tgt_items[e]) at e -- what
 *   lk_score_candidates writes --, d_tgt_ptr [n_rows + 1] ascends from 0 to total.  d_out [total]
 *   may be d_dots itself.  No panel is read.
 * ---------------------------------------------------------------------- */
#define LK_BMF_INVALID 0
#define LK_BMF_FOLD 1
#define LK_BMF_STORED 2
int lk_bmf_residual_rows(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                         const float *d_values, int64_t n_users, int64_t n_items,
                         int64_t n_queries, const int32_t *d_user_nums, const int64_t *d_out_ptr,
                         double global_bias, const float *d_item_biases, double damping_user,
                         double *d_out_ub, int32_t *d_out_indices, float *d_out_values,
                         void *stream);
int lk_bmf_finish_panel(float *d_panel, int64_t n_rows, int64_t n_items, int64_t ld,
                        const uint8_t *d_mode, const double *d_ub, double global_bias,
                        const float *d_item_biases, const int64_t *d_strike_ptr,
                        const int32_t *d_strike_items, void *stream);
int lk_bmf_finish_pairs(const float *d_panel, int64_t n_rows, int64_t n_items, int64_t ld,
                        const uint8_t *d_mode, const double *d_ub, double global_bias,
                        const float *d_item_biases, const int64_t *d_tgt_ptr,
                        const int32_t *d_tgt_items, int64_t first_entry, int64_t n_entries,
                        float *d_out, void *stream);
int lk_bmf_finish_ragged(const float *d_dots, int64_t n_rows, int64_t n_items,
                         const uint8_t *d_mode, const double *d_ub, double global_bias,
                         const float *d_item_biases, const int64_t *d_tgt_ptr,
                         const int32_t *d_tgt_items, int64_t total, float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * User-kNN scoring for a BATCH of queries.
 * Replaces `_accel.knn.user_score_items_explicit / _implicit(tgt_items, nbr_rows, nbr_sims,
 * ratings, max_nbrs, min_nbrs)` (src/accel/knn/user_score.rs:21-98): query q has neighbours
 * nbr_rows[nbr_ptr[q]..nbr_ptr[q+1]) (rows of the users x items ratings CSR, int64 offsets)
 * with similarities nbr_sims; every neighbour, in the given order, offers (weight = its
 * similarity, value = its rating) to the items it rated; per target item the `max_nbrs`
 * largest weights are kept (same ScoreAccumulator as item-kNN, accum.rs:16-239) and
 * score = sum(w * v) / sum(w)  (explicit)  or  sum(w)  (d_rat_values NULL: implicit);
 * fewer than min_nbrs contributors => NaN.  Negative neighbour rows / target items are nulls.
 * Workspace: lk_iknn_score_workspace_bytes(n_items, n_queries, max_nbrs).  Blocking.
 * ---------------------------------------------------------------------- */
int lk_uknn_score_batch(const int64_t *d_rat_indptr, const int32_t *d_rat_indices,
                        const float *d_rat_values, int64_t n_users, int64_t n_items,
                        int64_t n_queries, const int64_t *d_nbr_ptr, const int32_t *d_nbr_rows,
                        const float *d_nbr_sims, const int64_t *d_tgt_ptr,
                        const int32_t *d_tgt_items, int32_t max_nbrs, int32_t min_nbrs, void *d_ws,
                        float *d_out_scores, int32_t *d_out_counts, void *stream);

/* Neighbour similarities of user-kNN, `nbr_sims = user_vectors @ ratings`
 * (src/lenskit/knn/user.py:196) for a batch of dense query vectors:
 *   out[q][r] = sum over the entries (c, v) of CSR row r of  v * x[c][q]
 * x is [n_cols x ld_x] (column-major over queries: the queries' values of one item are
 * contiguous), out is [n_queries x ld_out].  Products accumulate in entry order (fmaf). */
int lk_csr_rows_dot(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                    const float *d_values, int64_t n_rows, const float *d_x, int64_t ld_x,
                    int64_t n_queries, float *d_out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------
 * User-kNN for whole PANELS of queries, every item scored (csrc/uknn_recommend.hip): what
 * `UserKNNScorer.__call__` (src/lenskit/knn/user.py:171-255) computes per query, as three
 * asynchronous calls on `stream`.
 * lk_uknn_query_panel: the dense query vectors of the histories d_hist_items[d_hist_ptr[q] ..
 *   d_hist_ptr[q + 1]) (int64 offsets; items outside [0, n_items) are skipped), item-major:
 *   x[item][q] (ld_x >= n_queries) = d_hist_ratings[e] - d_centre[q] (one f32 subtraction), or
 *   1.0 when d_hist_ratings is NULL (implicit feedback; d_centre is not read); absent items 0.
 *   A repeated item takes the value of its LAST occurrence (user.py:296-304's NumPy assignment).
 * lk_uknn_sims_panel: lk_csr_rows_dot with the output USER-major, out[user][q] (ld_out >=
 *   n_queries): the same fmaf chain over the stored row, the same bits.  d_self_user (may be
 *   NULL) [n_queries]: the query's own user, -1 = none; that entry is written as +0.0
 *   (user.py:192-194).
 * lk_uknn_score_panel: out[q][item] (ld_out >= n_items), ready for lk_argtopn.  The ratings come
 *   TRANSPOSED (lk_csr_transpose of the users x items matrix: items x users, int64 offsets, users
 *   ascending in a row; d_t_values NULL = implicit feedback).  A cell walks its item's row in
 *   stored order; every rater u with d_sims[u][q] >= thr (a NaN fails) offers (similarity,
 *   rating) to the cell's own ScoreAccumulator (accum.rs:16-239, step for step: a vector while it
 *   holds fewer than max_nbrs, then std's BinaryHeap, an entry displacing the minimum only when
 *   strictly greater).  Cell = sum(w * v) / sum(w) + d_offset[q] (explicit; d_offset NULL = 0)
 *   or sum(w) (implicit), sequential f32 sums in the accumulator's final array order, the product
 *   rounded before it is added; fewer than min_nbrs entries (or none): NaN.  max_col_len: the
 *   longest row of the transposed matrix (an accumulator is never given more slots than that;
 *   a smaller value than the truth gives wrong scores, never a stray store).  d_item_order (may
 *   be NULL) [n_items]: a permutation of the items, the order in which their tasks start
 *   (heaviest first).  mark_history as lk_slim_score_batch, on the histories d_hist_ptr /
 *   d_hist_items (may be NULL when 0): bit 0 turns the query's own items into NaN, bit 1 the
 *   whole row of a query without a known history item.  Workspace:
 *   lk_uknn_score_panel_workspace_bytes(max_nbrs, max_col_len) -- 0 (d_ws may be NULL) while
 *   min(max_nbrs, max_col_len) <= lk_uknn_score_panel_lds_max_nbrs(), the accumulators then live
 *   in LDS; above, in per-wave slabs of the workspace.  Every max_nbrs >= 1 is taken.
 * ---------------------------------------------------------------------- */
int lk_uknn_query_panel(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                        const float *d_hist_ratings, const float *d_centre, int64_t n_queries,
                        int64_t n_items, float *d_x, int64_t ld_x, void *stream);
int lk_uknn_sims_panel(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                       const float *d_values, int64_t n_users, const float *d_x, int64_t ld_x,
                       int64_t n_queries, const int32_t *d_self_user, float *d_out,
                       int64_t ld_out, void *stream);
int32_t lk_uknn_score_panel_lds_max_nbrs(void);
size_t lk_uknn_score_panel_workspace_bytes(int32_t max_nbrs, int64_t max_col_len);
int lk_uknn_score_panel(const int64_t *d_t_indptr, const int32_t *d_t_users,
                        const float *d_t_values, int64_t n_items, int64_t n_users,
                        int64_t max_col_len, const int32_t *d_item_order, const float *d_sims,
                        int64_t ld_sims, int64_t n_queries, float thr, int32_t max_nbrs,
                        int32_t min_nbrs, const float *d_offset, const int64_t *d_hist_ptr,
                        const int32_t *d_hist_items, int mark_history, void *d_ws, float *d_out,
                        int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------
 * User-kNN scores for the (query, target) PAIRS of a predict call (csrc/uknn_predict.hip).
 * Replaces, for a whole batch, `UserKNNScorer.__call__`'s scoring of the items it is asked for
 * (src/lenskit/knn/user.py:171-262), `user_score_items_explicit / _implicit`
 * (src/accel/knn/user_score.rs:21-98) and their `ScoreAccumulator` (src/accel/knn/accum.rs).
 * Query q of n_queries asks for the items d_tgt_items[d_tgt_ptr[q] .. d_tgt_ptr[q + 1]) (int64
 * offsets, ABSOLUTE entry numbers: d_tgt_ptr may be a slice of a longer array; a negative item
 * or one >= n_items is unknown); only entries in [first_entry, first_entry + n_entries) are read
 * and written.  d_out[entry] is what lk_uknn_score_panel writes into cell (q, item), bit for
 * bit: the item's row of the TRANSPOSED centred ratings (items x users, int64 offsets, users
 * ascending; d_t_values NULL = implicit feedback) walked in stored order, every rater u with
 * d_sims[q][u] >= thr (a NaN fails) offering (similarity, rating) to the cell's own accumulator
 * of max_nbrs entries, then sum(w * v) / sum(w) + d_offset[q] (explicit; d_offset NULL = 0) or
 * sum(w) (implicit), sequential f32 sums in the accumulator's final array order, the product
 * rounded before it is added; fewer than min_nbrs entries, none, or an unknown item: NaN.
 * d_sims: sims_user_major != 0: [n_users x ld_sims], ld_sims >= n_queries (lk_uknn_sims_panel's
 * output); 0: [n_queries x ld_sims], ld_sims >= n_users (lk_csr_rows_dot's).  d_self_user (may be
 * NULL) [n_queries]: the query's own user, -1 = none; that rater never passes (user.py:192-194
 * zeroes its similarity, and min_sim is positive), so the panel need not be touched.  max_col_len as for lk_uknn_score_panel.  Workspace:
 * lk_uknn_score_pairs_workspace_bytes(max_nbrs, max_col_len) -- 0 (d_ws may be NULL) while
 * min(max_nbrs, max_col_len) <= lk_uknn_score_pairs_lds_max_nbrs(), the accumulators then live
 * in LDS; above, in per-wave slabs of the workspace.  Every max_nbrs >= 1 is taken.  No atomics:
 * the same inputs give the same bits.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------- */
int32_t lk_uknn_score_pairs_lds_max_nbrs(void);
size_t lk_uknn_score_pairs_workspace_bytes(int32_t max_nbrs, int64_t max_col_len);
int lk_uknn_score_pairs(const int64_t *d_t_indptr, const int32_t *d_t_users,
                        const float *d_t_values, int64_t n_items, int64_t n_users,
                        int64_t max_col_len, const float *d_sims, int64_t ld_sims,
                        int sims_user_major, int64_t n_queries, const int32_t *d_self_user,
                        const int64_t *d_tgt_ptr,
                        const int32_t *d_tgt_items, int64_t first_entry, int64_t n_entries,
                        float thr, int32_t max_nbrs, int32_t min_nbrs, const float *d_offset,
                        void *d_ws, float *d_out, void *stream);

/* Device -> pageable host memory at PCIe speed: chunks through a ring of pinned staging slots,
 * a team of `n_threads` host threads (<= 14; 0 = 8) copies the landed chunks to `h_dst` in
 * parallel (first-touching its pages on many cores).  Used for results the reference hands
 * back as host arrays -- e.g. the similarity matrix of `compute_similarities`
 * (src/accel/knn/item_train.rs:86-91): SURVEY.md section 8d counts the kNN build "to CSR sim
 * matrix on host".  Blocking; waits for `stream` (the producer of `d_src`) first. */
int lk_download(void *h_dst, const void *d_src, size_t bytes, int32_t n_threads, void *stream);
/* The same for int32 values known to lie in [0, 65536) -- the column indices of a matrix with at
 * most 65 536 columns (ML-25M: 62 423 items): they cross PCIe as uint16 (narrowed on the device
 * into d_tmp_u16, n * 2 bytes) and the host team widens them back while it copies them into
 * h_dst, so the index half of a similarity matrix costs half the link time. */
/* Pin the staging ring of lk_download now (idempotent; otherwise the first large download pays). */
int lk_download_warmup(void);
int lk_download_i32_narrow(int32_t *h_dst, const int32_t *d_src, int64_t n, void *d_tmp_u16,
                           int32_t n_threads, void *stream);

/* ------------------------------------------------------------------------
 * EASE (`EASEScorer`, src/lenskit/knn/ease.py:88-147).
 * lk_ease_gram: the dense matrix the model inverts, G = X^T X + reg I for the binary
 *   users x items matrix X (`rates.co_occurrences("item", include_self=True, dense=True)` +
 *   the regularisation on the diagonal, ease.py:111-119; counting kernels
 *   src/accel/data/cooc.rs:47-192), from the off-diagonal co-occurrence counts in CSR form
 *   (the similarity build run on unit values, int64 offsets) and the item counts.
 * lk_ease_score_batch: `scores = q_vec @ self.weights` (ease.py:161-168) for a batch of
 *   queries: out[q][c] = sum over the history items i of query q of weights[i][c]
 *   (hist_items[hist_ptr[q]..hist_ptr[q+1]); items outside [0, n_items) are skipped).
 * ---------------------------------------------------------------------- */
int lk_ease_gram(const int64_t *d_cooc_indptr, const int32_t *d_cooc_indices,
                 const float *d_cooc_values, const int32_t *d_item_counts, int64_t n_items,
                 float reg, float *d_out, int64_t ld_out, void *stream);
int lk_ease_score_batch(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                        int64_t n_queries, const float *d_weights, int64_t n_items, int64_t ld_w,
                        float *d_out, int64_t ld_out, void *stream);
/* lk_ease_score_panel: the same sums as a panel for lk_argtopn, any number of queries: out[q][c] =
 *   the plain float32 sum, from zero and in history order, of weights[i][c] over the history
 *   items i of query q (items outside [0, n_items) -- -1 = unknown -- add nothing): the bits of
 *   lk_ease_score_batch.  The rows of d_weights need 4-byte alignment only (ld_w = n_items is odd
 *   in general).  mark_history as lk_slim_score_batch: bit 0 turns the query's own items into
 *   NaN, bit 1 the whole row of a query without a known item (0 otherwise). */
int lk_ease_score_panel(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                        int64_t n_queries, const float *d_weights, int64_t n_items, int64_t ld_w,
                        float *d_out, int64_t ld_out, int mark_history, void *stream);

/* ------------------------------------------------------------------------
 * Dense float32 GEMM and the blocked SPD inverse of EASE's training (csrc/spd_blocked.hip;
 * `_chol_invert_torch`, src/lenskit/knn/ease.py:190-208).
 * lk_gemm_f32: C <- beta C + alpha op(A) op(B) on row-major float32 matrices: C [m x n], op(A)
 *   [m x k], op(B) [k x n]; trans_a / trans_b != 0: the operand is stored transposed (A as
 *   [k x m], B as [n x k]).  Leading dimensions are in elements, at least the stored row length;
 *   pointers and rows need 4-byte alignment only; any m, n, k >= 0 (k = 0: C <- beta C).  A cell
 *   is the k-ordered fmaf chain of v_mfma_f32_32x32x2_f32 from zero, then fmaf(alpha, sum, beta c)
 *   -- alpha * sum when beta == 0, C is then not read.  No atomics, no split-k: a result's bits
 *   depend on its operands alone.  C must not overlap A or B.  tile_mask, in tiles of
 *   lk_gemm_tile() = 128 rows / columns counted from C's origin:
 *     LK_GEMM_LOWER       only the tiles on or below C's diagonal are computed, the others are
 *                         left untouched;
 *     LK_GEMM_K_FROM_COL  a tile's k starts at its first column (op(B) is lower triangular: zero
 *                         for k < the tile's columns);
 *     LK_GEMM_K_FROM_ROW  a tile's k starts at its first row (op(A) is upper triangular).
 * lk_spd_inverse_blocked: d_a [n x n, leading dimension ld] <- its inverse, in place, for a
 *   symmetric positive definite matrix (the lower triangle is read); the full result is written
 *   and is exactly symmetric.  Blocked Cholesky with block size 128: (a) right-looking
 *   factorisation, the diagonal blocks through lk_chol_upper_inverse (step = block + 1), panels
 *   and trailing updates through lk_gemm_f32; (b) the blocked inverse of the factor; (c) X^T X on
 *   the lower tiles, mirrored.  Every step is queued on `stream`; nothing waits for the host.
 *   d_work: lk_spd_inverse_blocked_workspace_bytes(n) bytes (a second n x n matrix, the diagonal
 *   blocks' inverses and a 128-row panel; 0 for an n that is not served).  n <=
 *   lk_spd_inverse_blocked_max_n() = 2^20, ld < 2^31.
 *   *d_flag (device) <- 0, or 1 + the number of the first block whose factorisation met a pivot
 *   that is not positive to working precision; every value stays finite on that path and the
 *   result is then all zeros.  The caller reads the flag once, after the call.
 * lk_spd_inverse_blocked_phases: the same with `phases` naming the steps to queue (bit 0 = (a),
 *   which also clears the flag, bit 1 = (b), bit 2 = (c); 7 = lk_spd_inverse_blocked): a timing
 *   hook -- three calls in that order on the same matrix and workspace are one inversion.
 * ---------------------------------------------------------------------- */
#define LK_GEMM_LOWER 1
#define LK_GEMM_K_FROM_COL 2
#define LK_GEMM_K_FROM_ROW 4
int32_t lk_gemm_tile(void);
int lk_gemm_f32(int trans_a, int trans_b, int64_t m, int64_t n, int64_t k, float alpha,
                const float *d_a, int64_t lda, const float *d_b, int64_t ldb, float beta,
                float *d_c, int64_t ldc, int tile_mask, void *stream);
int64_t lk_spd_inverse_blocked_max_n(void);
size_t lk_spd_inverse_blocked_workspace_bytes(int64_t n);
int lk_spd_inverse_blocked(float *d_a, int64_t n, int64_t ld, void *d_work, size_t work_bytes,
                           int32_t *d_flag, void *stream);
int lk_spd_inverse_blocked_phases(float *d_a, int64_t n, int64_t ld, void *d_work,
                                  size_t work_bytes, int32_t *d_flag, int phases, void *stream);

/* ------------------------------------------------------------------------
 * SLIM / fsSLIM (`SLIMScorer`, src/lenskit/knn/slim.py:53-152; csrc/slim.hip).
 * lk_slim_train_*: replaces `_accel.slim.train_slim(ui_matrix, iu_matrix, l1_reg, l2_reg,
 *   max_iters, max_nbrs)` (src/accel/slim/mod.rs:58-301): one elastic-net regression per target
 *   item by cyclic coordinate descent with soft thresholding, on the STRUCTURE of the users x
 *   items matrix `ui` and its transpose `iu` (offsets i32 / i64, both the same; no row may name a
 *   column twice).  Learns the rows of the TRANSPOSED weight matrix for the target items
 *   d_columns[0 .. n_cols) (NULL: every item, n_cols = n_items) -- rows in the order of the list,
 *   columns ascending, int64 offsets.  The result is the reference's bit for bit: the active list
 *   in first-encounter order, the fsSLIM cut (max_nbrs > 0: the max_nbrs largest cosines, float64
 *   key, stable) and its sorted order as the descent order, every coordinate's update a
 *   sequential float32 sum over the item's users in stored order, the stop at max |diff| <= 1e-3
 *   or after max_iters rounds, weights >= 1e-12 kept.  d_item_sqrt [n_items] = sqrt((double)
 *   user count of the item), made by the caller (NumPy's sqrt is correctly rounded).
 *   Two-phase like lk_iknn_build_*: _count trains the columns into a staging area of the
 *   workspace (lk_slim_train_workspace_bytes: n_cols x min(max_nbrs, n_items) pairs plus one
 *   slot per resident wave; cut long column lists into several calls), fills d_out_indptr
 *   [n_cols + 1] and returns the total through *h_total_nnz (blocking); _fill compacts the staging
 *   area into d_out_indices / d_out_values (same n_users, n_items, n_cols, max_nbrs, workspace).
 *   `ctl` (may be NULL): cancel / progress in columns; a cancelled _count returns LK_E_CANCELLED.
 *   h_stats (may be NULL) [3]: descent rounds, coordinate updates and residual entries summed by
 *   those updates, over all columns of the call.
 * lk_slim_score_batch: `x @ self.weights` (slim.py:139-144) for a batch of queries: out[q][c] =
 *   sum over the history items of query q, in history order, of weights[item][c] (the stored
 *   `weights` CSR, int64 offsets; a repeated history item counts twice, items outside
 *   [0, n_items) are skipped), every other cell 0.  mark_history prepares the panel for
 *   lk_argtopn: bit 0 turns the query's own items into NaN, bit 1 the whole row of a query whose
 *   history is empty.
 * lk_take_scores: out[r][k] = scores[r][idx[r][k]] (NaN where idx is negative): the scores of
 *   the lists lk_argtopn selected.
 * ---------------------------------------------------------------------- */
size_t lk_slim_train_workspace_bytes(int64_t n_users, int64_t n_items, int64_t n_cols,
                                     int64_t max_nbrs);
int lk_slim_train_count(const void *d_ui_indptr, const int32_t *d_ui_indices,
                        const void *d_iu_indptr, const int32_t *d_iu_indices, int indptr_is_64,
                        int64_t n_users, int64_t n_items, const double *d_item_sqrt, float l1_reg,
                        float l2_reg, int32_t max_iters, int64_t max_nbrs,
                        const int32_t *d_columns, int64_t n_cols, lk_task_ctl *ctl, void *d_ws,
                        int64_t *d_out_indptr, int64_t *h_total_nnz, int64_t *h_stats,
                        void *stream);
int lk_slim_train_fill(int64_t n_users, int64_t n_items, int64_t n_cols, int64_t max_nbrs,
                       const void *d_ws, const int64_t *d_out_indptr, int32_t *d_out_indices,
                       float *d_out_values, void *stream);
int lk_slim_score_batch(const int64_t *d_hist_ptr, const int32_t *d_hist_items, int64_t n_queries,
                        const int64_t *d_w_indptr, const int32_t *d_w_indices,
                        const float *d_w_values, int64_t n_items, float *d_out, int64_t ld_out,
                        int mark_history, void *stream);
int lk_take_scores(const float *d_scores, int64_t n_rows, int64_t row_len, const int32_t *d_idx,
                   int64_t n, float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Top-N lists from one shared order (`PopScorer.recommend_batch`; csrc/popular.hip): every
 * row's list is the same sorted item order with the row's own history skipped.
 * lk_shared_order_topn: d_order int32 [n_order] (item numbers, best first) and d_order_scores f32
 *   [n_order] (their scores, copied bit for bit).  List b = the first n entries of the order that
 *   do not occur in the history of row b, in order, written to d_out_idx / d_out_scores
 *   [n_rows x width], width = n (n < 0: n_order); positions past the end are -1 / NaN.  The
 *   history is a CSR of n_hist_rows rows (offsets int32 or int64, see hist_ptr_is_64) whose rows
 *   are in ascending item number; repeated entries are fine.  d_rows int32 [n_rows]: list b reads
 *   history row d_rows[b], -1 or out of range = no history (the plain first n); NULL: list b
 *   reads row b.  d_hist_ptr NULL: no list has a history.  One wave per list.
 * ---------------------------------------------------------------------- */
int lk_shared_order_topn(const int32_t *d_order, const float *d_order_scores, int64_t n_order,
                         const void *d_hist_ptr, int hist_ptr_is_64, const int32_t *d_hist_idx,
                         int64_t n_hist_rows, const int32_t *d_rows, int64_t n_rows, int64_t n,
                         int32_t *d_out_idx, float *d_out_scores, void *stream);

/* ------------------------------------------------------------------------
 * Association rules (`AssociationScorer`, src/lenskit/knn/association.py:59-163; csrc/assoc.hip).
 * The co-occurrence counts are the similarity build on unit values (lk_iknn_build_*, threshold
 * 0.5: `interact.co_occurrences("item")`, association.py:103).
 * lk_assoc_scale: the in-place scaling of association.py:110-124 on that CSR (int64 offsets):
 *   v = float32(double(count) / (double(item_counts[row]) + damping)); for LK_ASSOC_LIFT then
 *   v = v * float32(n_groups) in float32 and v = float32(double(v) / (double(item_counts[col]) +
 *   damping)) -- NumPy's `/=` by an int32 + float array and `*=` by a Python int, bit for bit.
 * lk_assoc_score_batch: `assoc_scores[ref_items, :].todense()` reduced over the rows
 *   (association.py:149-153) for a batch of queries, into a dense panel: for a query with m known
 *   reference items (items outside [0, n_items) are skipped, repeats count, order kept)
 *   LK_ASSOC_MEAN gives float32(double(s) / double(m)) with s the sequential float32 sum of the m
 *   cells in reference-item order (`np.mean(..., axis=0)`), LK_ASSOC_MAX their maximum; absent
 *   cells are 0.  No atomics: a query has the same bits alone or in any batch.  mark_history as
 *   lk_slim_score_batch: bit 0 turns the query's own items into NaN, bit 1 the whole row of a
 *   query without a known reference item (0 otherwise).  The panel is ready for lk_argtopn.
 * lk_assoc_window: the most item columns one workgroup accumulates (a test hook: item counts
 *   around its multiples take one more window).
 * ---------------------------------------------------------------------- */
#define LK_ASSOC_PROBABILITY 0
#define LK_ASSOC_LIFT 1
#define LK_ASSOC_MEAN 0
#define LK_ASSOC_MAX 1
int32_t lk_assoc_window(void);
int lk_assoc_scale(const int64_t *d_indptr, const int32_t *d_indices, float *d_values,
                   const int32_t *d_item_counts, int64_t n_items, int64_t n_groups, int method,
                   double damping, void *stream);
int lk_assoc_score_batch(const int64_t *d_ref_ptr, const int32_t *d_ref_items, int64_t n_queries,
                         const int64_t *d_s_indptr, const int32_t *d_s_indices,
                         const float *d_s_values, int64_t n_items, int reduce, float *d_out,
                         int64_t ld_out, int mark_history, void *stream);

/* Batched fold-in (new-user embeddings) -- `ImplicitMFScorer.new_user_embedding` /
 * `_train_new_row` (src/lenskit/als/_implicit.py:77-130) -- is the SAME algebra as one ALS
 * row with OtOr = Q^T Q + user_reg I: build a plan over the histories' CSR offsets and call
 * lk_als_implicit_half_epoch with `this` = the [n_queries x ld] output and `other` = Q. */

/* ------------------------------------------------------------------------
 * Stable CSR transpose on the device.
 * Replaces `_accel.data.transpose_csr(structure, permute)` (src/lenskit/_accel/data.pyi:12,
 * src/accel/data/transpose.rs:19-108; `SparseRowArray.transpose`, data/matrix.py:512-530):
 * out_indptr [n_cols+1] (same width as the input offsets), out_indices [nnz] = source rows,
 * out_perm [nnz] (same width; NULL = not wanted) = source entry position of every output
 * entry; inside an output row the input's entry order is kept (counting sort), so the
 * result equals the reference's entry for entry.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------- */
size_t lk_csr_transpose_workspace_bytes(int64_t nnz, int64_t n_cols, int indptr_is_64);
int lk_csr_transpose(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                     int64_t n_rows, int64_t n_cols, int64_t nnz, void *d_out_indptr,
                     int32_t *d_out_indices, void *d_out_perm, void *d_ws, size_t ws_bytes,
                     void *stream);

/* Relabelling of a CSR matrix on the device (set-up of the sharded ALS engine; the reference
 * builds both orientations on the host with SciPy, src/lenskit/als/_common.py:216-222):
 * output row r takes the entries of input row d_row_src[r] (-1: an empty padding row), every
 * column c becomes d_col_map[c]; the entry order inside a row is kept (NOT re-sorted by the new
 * column numbers: the row solve sums over a row's entries, any order).  d_out_indptr holds the
 * offsets of the result (same width as the input's), computed by the caller from the row
 * lengths; d_values / d_out_values may be NULL (structure only).  Asynchronous on `stream`. */
int lk_csr_relabel(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                   const float *d_values, int64_t n_rows_out, const int32_t *d_row_src,
                   const void *d_out_indptr, const int32_t *d_col_map, int32_t *d_out_indices,
                   float *d_out_values, void *stream);

/* Row gather of a CSR matrix on the device: the histories of a BATCH of queries cut out of the
 * training matrix in one launch.  Replaces, for a whole batch, the per-query
 * `UserTrainingHistoryLookup.__call__` -> `MatrixRelationshipSet.row_items`
 * (src/lenskit/basic/history.py:37-95) + the value vector of `ImplicitMFScorer.new_user_embedding`
 * (src/lenskit/als/_implicit.py:77-99: `ratings * weight`, or `np.full(n, weight)`), which the
 * reference's batch runner repeats query by query (src/lenskit/batch/_runner.py:283-308).
 * Output row r takes the entries of input row d_rows[r] (-1: an empty row) in their stored order;
 * d_out_indptr [n_rows_out + 1] (int64, the caller's prefix sums of the picked rows' lengths)
 * says where; out value = (d_values[e] - d_col_bias[column]) * scale in float32 (d_values NULL:
 * 1.0f in its place; d_col_bias NULL: nothing subtracted -- the item-kNN scorer mean-centres
 * the history ratings this way, src/lenskit/knn/item.py:268-271; d_out_values NULL: structure
 * only).  Asynchronous on `stream`. */
int lk_csr_gather_rows(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                       const float *d_values, int64_t n_rows_out, const int32_t *d_rows,
                       const int64_t *d_out_indptr, const float *d_col_bias, float scale,
                       int32_t *d_out_indices, float *d_out_values, void *stream);

/* ------------------------------------------------------------------------
 * Item-kNN rating normalisation (`ItemKNNScorer._center_ratings` / `_normalize_rows`,
 * src/lenskit/knn/item.py:202-228) on the ITEM-MAJOR matrix produced by lk_csr_transpose:
 *   lk_iknn_prep_center: c = r - means[item] (d_means NULL: implicit feedback, c = r),
 *       d_sumsq[item] = the |c|^2 of the item added one by one in entry (= user) order --
 *       the order of the reference's norm -- and *d_nonzero_flag = any |c| > 1e-8;
 *   lk_iknn_prep_scale: value = c * d_recip[item], written item-major and, through the
 *       transpose's permutation (same width as the offsets), user-major.
 * The per-item means (np.add.reduceat sums / counts) and recip = 1 / max(sqrt(sumsq),
 * FLT_MIN) are computed by the caller with the reference's own NumPy calls, which makes the
 * whole preparation bit-identical to the reference's.
 * ---------------------------------------------------------------------- */
int lk_iknn_prep_center(const void *d_item_indptr, int indptr_is_64, const float *d_item_values,
                        const float *d_means, int64_t n_items, float *d_centered,
                        float *d_sumsq, int32_t *d_nonzero_flag, void *stream);
int lk_iknn_prep_scale(const void *d_item_indptr, int indptr_is_64, const void *d_perm,
                       const float *d_centered, const float *d_recip, int64_t n_items,
                       float *d_item_values_out, float *d_user_values_out, void *stream);

/* ------------------------------------------------------------------------
 * Synthetic interaction matrix in HBM (bench tooling; SURVEY.md section 8d "cfg5 concrete
 * input": Philox-seeded, shard-wise on the device -- the reference has no counterpart, its
 * benchmarks read MovieLens files).  Given the row offsets d_indptr [n_rows+1] (int64; the
 * degrees are the caller's), row r receives exactly its degree DISTINCT items in ascending
 * order, item rank drawn ~ Zipf(1.0) from Philox4x32-10(key = seed, counter = (r, j)) and
 * duplicates pushed to the next free rank; any row range can be generated independently.
 * Rows longer than 32 entries (at most 4096) must be listed in d_long_rows. */
int lk_synth_zipf_rows(const int64_t *d_indptr, int64_t n_rows, int64_t n_items, uint64_t seed,
                       const int32_t *d_long_rows, int64_t n_long_rows, int32_t *d_out_indices,
                       void *stream);

/* ------------------------------------------------------------------------
 * Run evaluation (csrc/metrics.hip; lkpy_amd/metrics.py composes the metric values on the host
 * from these statistics with the reference's own expressions).  Replaces the per-list loop of
 * `MeasurementCollector.add_collection_measurements` (src/lenskit/metrics/_collect.py:156-186)
 * and the `measure_list` bodies it calls.  Item NUMBERS throughout; a truth CSR has one row per
 * list (int64 offsets, items ascending, no duplicates) -- rows cut out of the per-test-set
 * matrix with lk_csr_gather_rows.  All calls are asynchronous on `stream`; every float64 output
 * is a sum taken in rank (list) order and depends on its own list and truth row only.
 *
 * lk_rank_stats: d_lists [n_lists x ld] in rank order, the first `len` columns are read; entries
 *   < 0 are dropped BEFORE ranks are assigned (rank = 1 + kept entries before it).  `cutoffs`
 *   (host, 1..8 values, 0 = whole list), d_weights [n_tables x w_ld] float64 with
 *   d_weights[t * w_ld + rank - 1] = w_t(rank), w_ld >= len, 0..4 tables, and
 *   n_cutoffs * (1 + 2 n_tables) <= 64.  Outputs (field-major):
 *     d_out_counts int32 [(2 + 2 n_cutoffs) x n_lists]: row 0 n_recs (kept entries), row 1 the
 *       truth row's length, rows 2 + 2c / 3 + 2c: n_hits (`recs.isin(test).sum()`, a repeated
 *       item counts each time) and first_hit (1-based rank, 0 = none) inside cutoff c
 *       (ranking/_pr.py:44,67, _hit.py:42, _recip.py:45-50);
 *     d_out_sums float64 [n_cutoffs * (1 + 2 n_tables) x n_lists]: per cutoff c, row
 *       c * (1 + 2 n_tables) = ap_sum, sum over hit ranks of (hits up to here) / rank
 *       (_map.py:37-41); + 1 + 2t = w_hits, sum of w_t(rank) over hit ranks (`_binary_dcg`,
 *       _dcg.py:248-255; `rank_biased_precision`, _rbp.py:17-37); + 2 + 2t = g_hits, sum of
 *       max(gain, 0) * w_t(rank), the float32 gain widened first, a NaN gain skipped
 *       (`_graded_dcg`, _dcg.py:224-245; 0 when d_truth_gains is NULL).
 * lk_ideal_gain: graded NDCG's denominator (_dcg.py:118-133).  Per truth row the gains with NaN
 *   dropped and negatives clipped to 0, sorted descending; for combination k the first
 *   cutoffs[k] of them (0: all) times w_tables[k](1 ..) added in that order:
 *   d_out_ideal [n_combos x n_rows]; d_out_count [n_rows] = non-NaN gains.  Rows longer than
 *   4096 entries must be listed in d_long_rows and are sorted in d_ws
 *   (lk_ideal_gain_workspace_bytes(n_long_rows, longest_row)); products beyond w_ld are not
 *   formed.
 * lk_predict_errors: RMSE / MAE (predict.py:73-111, 131-137, 164-169).  Ragged prediction lists
 *   of DISTINCT items (int64 offsets, item numbers, float32 scores) against the truth CSR with float32 ratings, or -- with
 *   d_truth_ptr NULL -- against d_pred_ratings carried by the lists.  e = score - rating, e * e
 *   and |e| in float32, accumulated in float64 in list order.  d_out_sums [2 x n_lists]: sse,
 *   sae; d_out_counts [3 x n_lists]: n (finite errors), n_missing_score (rated, not scored or
 *   scored NaN), n_missing_truth (scored, no rating) -- predict.py:102-109.
 * ---------------------------------------------------------------------- */
int lk_rank_stats(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                  const int64_t *d_truth_ptr, const int32_t *d_truth_items,
                  const float *d_truth_gains, const int32_t *cutoffs, int32_t n_cutoffs,
                  const double *d_weights, int32_t n_tables, int64_t w_ld, int32_t *d_out_counts,
                  double *d_out_sums, void *stream);
size_t lk_ideal_gain_workspace_bytes(int64_t n_long_rows, int64_t longest_row);
int lk_ideal_gain(const int64_t *d_truth_ptr, const float *d_gains, int64_t n_rows,
                  const int32_t *d_long_rows, int64_t n_long_rows, int64_t longest_row,
                  void *d_ws, const int32_t *cutoffs, const int32_t *tables, int32_t n_combos,
                  const double *d_weights, int32_t n_tables, int64_t w_ld, double *d_out_ideal,
                  int32_t *d_out_count, void *stream);
int lk_predict_errors(int64_t n_lists, const int64_t *d_pred_ptr, const int32_t *d_pred_items,
                      const float *d_pred_scores, const float *d_pred_ratings,
                      const int64_t *d_truth_ptr, const int32_t *d_truth_items,
                      const float *d_truth_ratings, double *d_out_sums, int32_t *d_out_counts,
                      void *stream);

/* ------------------------------------------------------------------------
 * Exposure, diversity, popularity and reranking metrics (csrc/diversity.hip; the values are
 * composed on the host by lkpy_amd/metrics.py and lkpy_amd/reranking_metrics.py).  Item NUMBERS
 * throughout.  Lists are the dense int32 [n_lists x ld] panels of lk_rank_stats: the first `len`
 * columns are read, entries < 0 are dropped BEFORE ranks are assigned, `cutoff` keeps the ranks
 * <= cutoff (0 = whole list); an item number >= n_items is an UNKNOWN item: it keeps its rank.
 * A rank-weight table is float64 with d_weights[rank - 1] = w(rank), w_ld >= the longest kept
 * list; NULL = every weight is 1.  All calls are asynchronous on `stream`, wave64, no float
 * atomics; a product and the sum it enters are two roundings.
 *
 * lk_item_exposure: d_totals[item] += w(rank) over every kept known entry inside the cutoff
 *   (`GiniAccumulator.add`, ranking/_gini.py:127-129, with the weights of `ListGini` /
 *   `ExposureGini.measure_list`, _gini.py:72-75, 112-116).  d_totals float64 [n_items] is
 *   accumulated ONTO; an item's additions happen in list order, then rank order, as ONE chain
 *   that starts at the value already there: the result is bit-identical to
 *   `for list in lists: totals[items] += weights` and to the same lists fed in several calls.
 *   d_ws: lk_item_exposure_workspace_bytes(n_lists, len) bytes (a stable radix sort of
 *   item -> entry, then one wave per item walks its run).
 * lk_list_category_stats: the item x category matrix as CSR (int64 offsets [n_items + 1], int32
 *   columns without duplicates inside a row, float64 values), n_cats <= lk_list_category_max()
 *   (7168: the column sums s_c = sum_i w_i M[item_i, c] of a list live in LDS, 8 bytes each).
 *   s_c is added over the known kept items in rank order, w_i the weight of the item's own rank:
 *   bit-identical to a sequential float64 column sum of `matrix * weights[:, None]`
 *   (ranking/_entropy.py:78-81).  d_out_known int32 [n_lists]: known items inside the cutoff;
 *   d_out_stats float64 [3 x n_lists]: sq_sum = sum_c s_c^2, self_sum = sum_i sum_c M[i, c]^2
 *   (with unit weights sum_{i<j} v_i . v_j = (sq_sum - self_sum) / 2: `intra_list_similarity`,
 *   ranking/_ils.py:39-44), entropy = -sum_c p_c log2 p_c, p = (s + 1e-6) / sum(s + 1e-6)
 *   (`matrix_column_entropy`, _entropy.py:81-86).
 * lk_list_gather_mean: d_out_sum[list] = sum, in rank order, of d_table[item] (float64
 *   [n_items]) over the kept entries inside the cutoff, an unknown item adding 0;
 *   d_out_len[list] = those entries, unknown ones included (`MeanPopRank.measure_list`,
 *   ranking/_pop.py:77-84).
 * lk_list_pair_stats: ragged lists (int64 offsets, item numbers >= 0, distinct inside a list):
 *   pair q is reference list d_a_rows[q] (q itself when d_a_rows is NULL; < 0 = no reference
 *   list, treated as an empty one) and reranked list q.  Depth 1 <= n <= 1024, d_weights
 *   float64 [n].  d_out_rbo[q] = sum_{d=1..n} (overlap_d / d) * w_d with overlap_d =
 *   |a[:d] & b[:d]|, added sequentially in d (reranking/_rbo.py:45-55; the host divides by the
 *   total weight); d_out_lip[q] = max(n, largest 0-based position in a of an item of b[:n]) - n
 *   and d_out_flag[q] = 1 where a is empty (reranking/_lip.py:37-48).  a is scanned once.
 * ---------------------------------------------------------------------- */
int32_t lk_list_category_max(void);
size_t lk_item_exposure_workspace_bytes(int64_t n_lists, int64_t len);
int lk_item_exposure(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                     int32_t cutoff, const double *d_weights, int64_t w_ld, int32_t n_items,
                     double *d_totals, void *d_ws, void *stream);
int lk_list_category_stats(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                           int32_t cutoff, int32_t n_items, const int64_t *d_cat_ptr,
                           const int32_t *d_cat_cols, const double *d_cat_vals, int32_t n_cats,
                           const double *d_weights, int64_t w_ld, int32_t *d_out_known,
                           double *d_out_stats, void *stream);
int lk_list_gather_mean(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                        int32_t cutoff, const double *d_table, int32_t n_items,
                        double *d_out_sum, int32_t *d_out_len, void *stream);
int lk_list_pair_stats(int64_t n_pairs, const int32_t *d_a_rows, const int64_t *d_a_ptr,
                       const int32_t *d_a_items, const int64_t *d_b_ptr, const int32_t *d_b_items,
                       int32_t n, const double *d_weights, double *d_out_rbo, int32_t *d_out_lip,
                       int32_t *d_out_flag, void *stream);

/* ------------------------------------------------------------------------
 * FlexMF implicit (csrc/flexmf.hip): the minibatch trainer of `lenskit.flexmf.FlexMFImplicitScorer`
 * -- score = b_u + b_i + p_u . q_i, logistic / pairwise (BPR) / WARP loss, AdamW or SparseAdam.
 * All tables are float32, row-major and UNPADDED ([rows x k], biases [rows]); a NULL bias table
 * is an absent one (counts as 0).  Every call is asynchronous on `stream`; nothing is atomic
 * on floats and every sum has a fixed order, so a step is a function of its inputs alone.
 * ---------------------------------------------------------------------- */
#define LK_FLEXMF_LOGISTIC 0
#define LK_FLEXMF_PAIRWISE 1
#define LK_FLEXMF_WARP 2
#define LK_FLEXMF_ADAMW 0
#define LK_FLEXMF_SPARSE_ADAM 1
#define LK_FLEXMF_MAX_K 256

/* table order everywhere: 0 u_embed, 1 i_embed, 2 u_bias, 3 i_bias (`FlexMFModel`,
 * src/lenskit/flexmf/_model.py:73-81) with the optimiser's two moment tables of each */
typedef struct lk_flexmf_tables {
    float *param[4];
    float *exp_avg[4];
    float *exp_avg_sq[4];
    int64_t n_users, n_items;
    int32_t k;
} lk_flexmf_tables;

typedef struct lk_flexmf_hyper {
    int32_t loss;      /* LK_FLEXMF_LOGISTIC | PAIRWISE | WARP */
    int32_t optimizer; /* LK_FLEXMF_ADAMW | LK_FLEXMF_SPARSE_ADAM */
    int32_t l2;        /* 1: the explicit L2 term of reg_method = "L2" */
    int32_t n_neg;     /* negatives per positive */
    /* doubles, as Torch's optimisers hold them: each is rounded to float32 where Torch rounds */
    double pos_weight; /* logistic loss only */
    double reg;        /* weight decay (AdamW) or the L2 strength */
    double lr, beta1, beta2, eps;
    double bias_corr1, bias_corr2; /* 1 - beta^t of the step about to be taken, from the host */
} lk_flexmf_hyper;

/* Negative sampling -- `sample_negatives` (src/accel/data/sampling.rs:17-63) behind
 * `MatrixRelationshipSet.sample_negatives` (src/lenskit/data/_relationships.py:725-793).
 * d_out [n_rows x n]: for (row r, replicate j) a column drawn uniformly from [0, n_cols)
 * (popular: the column of a uniformly drawn entry of d_indices), redrawn while it is an entry of
 * CSR row d_rows[r] (binary search; columns ascending inside a row), at most max_attempts
 * times, after which the last draw stands; verify = 0: the first draw stands.  The draw is
 * Philox4x32-10(key, (counter, r, j, attempt)): the reference's PCG64 stream is not reproduced,
 * the contract is distributional. */
int lk_flexmf_sample_negatives(const int64_t *d_indptr, const int32_t *d_indices, int64_t nnz,
                               int64_t n_cols, const int32_t *d_rows, int64_t n_rows, int32_t n,
                               int popular, int verify, int32_t max_attempts, uint64_t key,
                               uint64_t counter, int32_t *d_out, void *stream);

/* One batch's (user, item) pairs: out[i] = all[perm[i]] for both arrays -- `make_batch`
 * (src/lenskit/flexmf/_training.py:350-358) on the device-resident epoch permutation. */
int lk_flexmf_gather_batch(const int32_t *d_perm, int64_t n, const int32_t *d_all_users,
                           const int32_t *d_all_items, int32_t *d_users, int32_t *d_items,
                           void *stream);

/* The WARP / "misranked" negative search -- `FlexMFWARPTrainer.scored_negatives`
 * (src/lenskit/flexmf/_implicit.py:293-396) -- as a function of a candidate table
 * d_cand [batch x tries]: per sample, try t = 1.. takes candidate t - 1; a candidate scoring
 * strictly above the best so far replaces it (count = t); the search stops once best >= the
 * positive's score.  Candidates are scored only up to the stopping try.  Outputs: d_neg [batch],
 * d_count [batch] int32, d_weight [batch] float64 = the harmonic-number approximation at
 * rank = (n_items - 1) / (count + 1), in double. */
int lk_flexmf_warp_search(const lk_flexmf_tables *tables, const int32_t *d_users,
                          const int32_t *d_pos, const int32_t *d_cand, int64_t batch,
                          int32_t tries, int32_t *d_neg, int32_t *d_count, double *d_weight,
                          void *stream);

/* One training step -- `FlexMFImplicitTrainer.train_batch` + `opt.step()`
 * (src/lenskit/flexmf/_implicit.py:253-274,399-415, _model.py:145-198, _training.py:238-252):
 * forward, loss, gradients, per-row gradient sums (stable radix sort by destination row, then
 * one wave per touched row adding in sample order) and the optimiser update, as
 * torch.optim.AdamW / torch.optim.SparseAdam perform it.  d_neg [batch x n_neg];
 * d_weights [batch] float64 (WARP only).  d_slot: int32 [n_users + n_items], all -1 on entry and
 * on return (AdamW only; NULL otherwise).  *d_loss receives the batch loss, *d_loss_sum (may be
 * NULL) has it added. */
size_t lk_flexmf_step_workspace_bytes(int64_t batch, int32_t n_neg, int32_t k);
int lk_flexmf_step(const lk_flexmf_tables *tables, const lk_flexmf_hyper *hyper,
                   const int32_t *d_users, const int32_t *d_pos, const int32_t *d_neg,
                   const double *d_weights, int64_t batch, void *d_ws, int32_t *d_slot,
                   float *d_loss, float *d_loss_sum, void *stream);

/* ------------------------------------------------------------------------
 * FlexMF explicit (csrc/flexmf.hip): the trainer of `lenskit.flexmf.FlexMFExplicitScorer`
 * (src/lenskit/flexmf/_explicit.py:25-125) -- the same tables and optimisers, a rating per
 * sample, squared error, no negatives.
 * ---------------------------------------------------------------------- */
#define LK_FLEXMF_MSE 3 /* lk_flexmf_hyper.loss of lk_flexmf_step_explicit */

/* out[i] = all[perm[i]] of a float32 array: the ratings' companion of lk_flexmf_gather_batch
 * (`make_batch` with `fields`, src/lenskit/flexmf/_training.py:350-358). */
int lk_flexmf_gather_values(const int32_t *d_perm, int64_t n, const float *d_all, float *d_out,
                            void *stream);

/* One training step -- `FlexMFExplicitTrainer.train_batch` + `opt.step()`
 * (src/lenskit/flexmf/_explicit.py:108-125, _model.py:145-198, _training.py:238-252).
 * hyper->loss = LK_FLEXMF_MSE, hyper->n_neg = 0, pos_weight is ignored.  With
 * pred = b_u + b_i + p_u . q_i and B = batch: the loss is mean (pred - r)^2 and *d_loss receives
 * it WITHOUT the L2 term (the reference returns `loss`, not `loss_all`); each sample's score
 * gradient is 2 (pred - r) / B.  hyper->l2 = 1 (reg_method "L2", the explicit default) adds
 * reg * mean(b_u^2 + b_i^2 + |p_u| + |q_i|) -- norms, not squared norms -- to the objective: per
 * occurrence in the batch reg x / (B |x|) to an embedding row x (0 where |x| = 0, as Torch
 * gives) and 2 reg b / B to a bias, the same on the user and the item side (the implicit step
 * halves the item side).  Optimiser, staging, the float64 per-row sums in sample order, d_slot
 * and d_loss_sum: as lk_flexmf_step.  d_ratings: float32 [batch].  A batch may hold a user, or
 * a (user, item) pair, any number of times.  The workspace has its own size function because
 * lk_flexmf_step_workspace_bytes rejects n_neg = 0. */
size_t lk_flexmf_step_explicit_workspace_bytes(int64_t batch, int32_t k);
int lk_flexmf_step_explicit(const lk_flexmf_tables *tables, const lk_flexmf_hyper *hyper,
                            const int32_t *d_users, const int32_t *d_items,
                            const float *d_ratings, int64_t batch, void *d_ws, int32_t *d_slot,
                            float *d_loss, float *d_loss_sum, void *stream);

/* ------------------------------------------------------------------------
 * Ragged pair scoring for factor models (csrc/mf_pairs.hip): d_out[t] = the inner product over
 * k columns of row d_user_rows[q] of d_users with row d_tgt_items[t] of d_items, for every t in
 * [d_tgt_ptr[q], d_tgt_ptr[q + 1]) -- `FlexMFScorerBase.__call__`
 * (src/lenskit/flexmf/_base.py:116-164) for n_queries queries in one launch, without a row of
 * scores per user.  The operands are the padded matrices of lk_score_dense (leading dimensions
 * multiples of 4 floats covering k rounded up to 4, bases 16-byte aligned).  d_tgt_ptr: int64
 * [n_queries + 1], ascending from 0 to total.  A user row or a target outside its table (-1:
 * unknown) gives NaN.  The summation order depends on k alone, so a score has the same bits
 * whatever else the batch holds; no atomics.
 * ---------------------------------------------------------------------- */
int lk_mf_score_pairs(const float *d_users, int32_t ld_users, int64_t n_users,
                      const float *d_items, int32_t ld_items, int64_t n_items, int32_t k,
                      const int32_t *d_user_rows, int64_t n_queries, const int64_t *d_tgt_ptr,
                      const int32_t *d_tgt_items, int64_t total, float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Per-query candidate lists (csrc/candidates.hip): scoring and ranking "these items for this
 * query" for a batch -- `BatchRecRequest.candidates` (src/lenskit/batch/_queries.py:50-78),
 * `pipe.run("recommender", query=, items=, n=)` and `BatchPipelineRunner.score`
 * (src/lenskit/batch/_runner.py:114-124).  One ragged layout throughout: d_tgt_ptr int64
 * [n_queries + 1] ascending from 0 to total, d_tgt_items int32 [total]; the caller validates the
 * offsets on the host, the kernels clamp them and range-check every item number and user row
 * before it becomes an address.  No atomics; a result depends on its own query alone.
 *
 * lk_score_candidates: the signature and operands of lk_mf_score_pairs (leading dimensions
 *   multiples of 4 floats covering k rounded up to 4, bases 16-byte aligned, k in 1..1024), but
 *   d_out[t] is the SINGLE chain acc = 0; for f = 0 .. k-1: acc = fmaf(u[f], q[f], acc) -- the
 *   chain of lk_score_dense / lk_score_topk, so d_out[t] has the bits of that panel's entry
 *   (user row, item) for every k.  A user row or an item outside its table (-1: unknown) gives
 *   NaN.  total = 0 returns without a launch.
 * lk_panel_take_ragged: d_out[t] = d_panel[q * ld + d_tgt_items[t]] for t in query q's range (NaN
 *   for an item outside [0, n_items)): lk_take_scores for ragged targets, the bridge from any
 *   [n_queries x ld] score panel.
 * lk_ragged_topn: lk_argtopn applied to every segment of d_scores f32 [total]: entries with a NaN
 *   score or a negative item number are dropped, the rest descend in the order of the selection
 *   kernel's keys (-0.0 ties with +0.0, +-inf are valid), ties go to the lower position in the
 *   segment; repeated item numbers are separate entries.  d_out_idx int32 / d_out_score f32
 *   [n_queries x width]: item NUMBERS and the input scores' own bits, padded with -1 / NaN.
 *   width = n, or with n < 0 width = max_len and every valid entry is ranked.  max_len: the
 *   longest segment, from the caller's host copy of the offsets (a segment longer than that is
 *   not ranked).  Segments of at most lk_ragged_topn_wave_max() (64) entries take one wave, up to
 *   lk_ragged_topn_block_max() (1024) one workgroup with the keys in LDS; when max_len is larger
 *   the batch is sorted once (stable radix sort of (query, key)) and the long segments are
 *   emitted from that -- d_ws then needs lk_ragged_topn_workspace_bytes(total, max_len) bytes
 *   (0 otherwise).  total < 2^31 per call; no other limit on n or the segment length.
 * ---------------------------------------------------------------------- */
int lk_score_candidates(const float *d_users, int32_t ld_users, int64_t n_users,
                        const float *d_items, int32_t ld_items, int64_t n_items, int32_t k,
                        const int32_t *d_user_rows, int64_t n_queries, const int64_t *d_tgt_ptr,
                        const int32_t *d_tgt_items, int64_t total, float *d_out, void *stream);
int lk_panel_take_ragged(const float *d_panel, int64_t n_queries, int64_t n_items, int64_t ld,
                         const int64_t *d_tgt_ptr, const int32_t *d_tgt_items, int64_t total,
                         float *d_out, void *stream);
int32_t lk_ragged_topn_wave_max(void);
int32_t lk_ragged_topn_block_max(void);
size_t lk_ragged_topn_workspace_bytes(int64_t total, int64_t max_len);
int lk_ragged_topn(int64_t n_queries, const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                   const float *d_scores, int64_t total, int32_t n, int64_t max_len, void *d_ws,
                   int32_t *d_out_idx, float *d_out_score, void *stream);

/* ------------------------------------------------------------------------
 * Per-query candidate lists over a sparse item-item model (csrc/sparse_candidates.hip): the
 * entries of the lk_slim_score_batch / lk_assoc_score_batch panel at ragged targets, computed
 * without the panel.
 *   history  d_hist_ptr int64 [n_hist_rows + 1], d_hist_items int32 [hist_nnz] (-1: unknown item).
 *            d_rows int32 [n_queries]: query q reads history row d_rows[q] (a row number outside
 *            [0, n_hist_rows), -1 say, is a query without history); NULL: query q reads row q.
 *   model    d_m_indptr int64 [n_items + 1], d_m_indices int32 [model_nnz] ascending and without
 *            repeats inside a row, d_m_values f32 [model_nnz].
 *   targets  the ragged layout of lk_score_candidates.
 * d_out[t], for target column c = d_tgt_items[t] of query q: walk q's history in the order
 * stored, skip the items outside [0, n_items), count every other one in m (repeats included), and
 * where the item's model row holds column c fold its value v into an accumulator that starts at
 * 0.f -- one plain float32 operation per history item, in history order:
 *   LK_SPARSE_SUM   acc = acc + v; NaN for a history without entries, else acc (0.0 for a
 *                   non-empty history without a known item) -- the cell of lk_slim_score_batch
 *   LK_SPARSE_MEAN  acc = acc + v; NaN for m = 0, else float32(double(acc) / double(m))
 *   LK_SPARSE_MAX   acc = fmaxf(acc, v): absent cells count as 0; NaN for m = 0
 *                   (both: the cell of lk_assoc_score_batch)
 * A target outside [0, n_items) gives NaN.  Every offset is clamped to its array and every row
 * and item number range-checked before it becomes an address.  total = 0 returns without a
 * launch.  No atomics; a result depends on its own query's history and its own target alone.
 * ---------------------------------------------------------------------- */
#define LK_SPARSE_SUM 0
#define LK_SPARSE_MEAN 1
#define LK_SPARSE_MAX 2
int lk_sparse_score_candidates(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                               int64_t n_hist_rows, int64_t hist_nnz, const int32_t *d_rows,
                               int64_t n_queries, const int64_t *d_m_indptr,
                               const int32_t *d_m_indices, const float *d_m_values,
                               int64_t n_items, int64_t model_nnz, const int64_t *d_tgt_ptr,
                               const int32_t *d_tgt_items, int64_t total, int reduce,
                               float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Stochastic top-N ranking (csrc/stochastic.hip): the sort keys of
 * `StochasticTopNRanker._compute_keys` (src/lenskit/stochastic/_ranker.py:119-156) for a panel
 * of score rows; lk_argtopn of a key row is one Plackett-Luce sample, lk_take_scores its keys
 * (replacing `valid_items.top_n(n, scores=keys)`, _ranker.py:113-117).
 *   x = score * scale (_ranker.py:123).  Only finite scores outside the row's exclusion CSR row
 *   (int64 offsets, int32 ascending items, as lk_score_topk takes it; NULL: none) take part --
 *   `valid_mask`, _ranker.py:104-105; N = their count.
 *   transform  LK_STOCHASTIC_SOFTMAX: log w = x - max - log sum exp(x - max)   (_ranker.py:140-144)
 *              LK_STOCHASTIC_LINEAR:  w = t / sum t, t = (x - min) / (max - min); w = 1 / N when
 *                                     max == min or the sum is 0                (_ranker.py:125-139)
 *              LK_STOCHASTIC_NONE:    w = x                                     (_ranker.py:145-146)
 *   key        g = max(log w, log FLT_MIN) - log(-log u).  The reference's key
 *              log(u) / max(w, FLT_MIN) (_ranker.py:149-153) is -exp(-g): the same order, kept in
 *              the log domain because its float32 value is -inf for every weight on the clamp.
 *   u          Philox4x32-10 with key `seed` and counter (item >> 2, sample, stream lo, stream hi);
 *              word (item & 3) = b gives u = (2 (b >> 9) + 1) 2^-24.  A draw depends on (seed,
 *              stream, sample, item number) only.
 * lk_stochastic_row_stats: d_stats [n_rows x 4] = max x, min x, the sum (of exp(x - max), of t, 0
 *   for NONE) as float32 and N as int32, per row.  One pass shared by every sample of a call.
 * lk_stochastic_keys: d_keys [n_rows x ld_keys] = g, NaN for the entries that take no part
 *   (lk_argtopn skips them).  d_streams: uint64 [n_rows].
 * lk_stochastic_key_of_bits: d_out[i] = max(d_log_weight[i], log FLT_MIN) - log(-log u(d_bits[i])),
 *   the key function on given random words (tests: both ends of u).
 * Reductions run in an order fixed by row_len alone and use no atomics: a row has the same stats
 * and keys alone, in any batch, at any leading dimension.
 * ---------------------------------------------------------------------- */
#define LK_STOCHASTIC_NONE 0
#define LK_STOCHASTIC_SOFTMAX 1
#define LK_STOCHASTIC_LINEAR 2
int lk_stochastic_row_stats(const float *d_scores, int64_t n_rows, int64_t row_len, int64_t ld,
                            const int64_t *d_excl_ptr, const int32_t *d_excl_items,
                            int32_t transform, float scale, float *d_stats, void *stream);
int lk_stochastic_keys(const float *d_scores, int64_t n_rows, int64_t row_len, int64_t ld,
                       const int64_t *d_excl_ptr, const int32_t *d_excl_items, int32_t transform,
                       float scale, const float *d_stats, uint64_t seed,
                       const uint64_t *d_streams, uint32_t sample, float *d_keys, int64_t ld_keys,
                       void *stream);
int lk_stochastic_key_of_bits(const float *d_log_weight, const uint32_t *d_bits, int64_t n,
                              float *d_out, void *stream);

/* ------------------------------------------------------------------------
 * The same keys for ragged candidate lists (csrc/ragged_stochastic.hip).  Segment s -- the entries
 * d_ptr[s] .. d_ptr[s + 1] - 1 (int64 [n_segments + 1], ascending from 0 to total) -- is the row of
 * a [1 x d_width[s]] panel that holds d_scores[t] at column d_addr[t] and NaN everywhere else:
 *   d_stats [n_segments x 4]  the bits lk_stochastic_row_stats writes for that row;
 *   d_keys [samples x total]  d_keys[j * total + t] = the bits lk_stochastic_keys writes at column
 *                             d_addr[t] for sample first_sample + j and stream d_streams[s]; NaN
 *                             for an entry with a non-finite score.
 * One statistics pass serves every sample.  CONTRACT: the addresses of a segment ascend strictly
 * and lie in [0, d_width[s]) -- the float32 sum is added in the panel kernel's tree (entry t
 * belongs to its thread (d_addr[t] >> 2) % BLK, BLK = 64 for a width <= 2048 and 256 above), which
 * a walk in address order reproduces.  The caller checks that on its host copy; the kernel uses
 * no input as a memory address (offsets are clamped to [0, total], an address outside its row
 * takes no part), so a broken contract gives other bits, never an access out of bounds.
 * One wave per segment; a segment longer than lk_ragged_stochastic_chunk() (512) entries is
 * walked in chunks of that many by the same wave.  No atomics: a segment has the same bits alone
 * and inside any batch.  total < 2^31.
 * ---------------------------------------------------------------------- */
int32_t lk_ragged_stochastic_chunk(void);
int lk_ragged_stochastic_keys(int64_t n_segments, const int64_t *d_ptr, const int32_t *d_addr,
                              const float *d_scores, int64_t total, const int32_t *d_width,
                              const uint64_t *d_streams, int32_t transform, float scale,
                              uint64_t seed, uint32_t first_sample, int32_t samples,
                              float *d_stats, float *d_keys, void *stream);

/* ------------------------------------------------------------------------
 * FA*IR top-N reranking (csrc/fair.hip): the greedy loop of `FAIRReranker.__call__`
 * (src/lenskit/reranking/fair.py:198-248) for a batch of ranked lists, a wave per list.
 *   d_lists        int32 [n_rows x ld], row_len entries of a row are looked at: item numbers in list
 *                  order.  d_lengths (int32 [n_rows], clamped to 0..row_len) gives each row's
 *                  length; NULL: a row ends at its first negative entry (trailing -1 padding).
 *                  With lengths a negative entry inside a row is an item unknown to the vocabulary.
 *   d_scores       float32 in the layout of d_lists, or NULL; copied as bits, never computed with.
 *   d_is_protected uint8 [n_items]: non-zero = protected.  An item number outside 0..n_items-1
 *                  is unprotected and stays in the list (fair.py:202-205).
 *   d_m_table      int32 [n_table]: slot i needs m[i] protected items among slots 0..i (`m_list`,
 *                  fair.py:176); n_table <= LK_FAIR_MAX_N (the kernel's LDS queues: 12 n_out bytes
 *                  per row), n_out <= n_table.
 *   outputs        d_out_items [n_rows x n_out] (-1 past min(n_out, length)), d_out_scores (NaN
 *                  past it; NULL, or with d_scores) and d_out_pos (NULL or the slot's position in
 *                  its input row, -1 past it), all dense.
 * With P / U the positions of the protected / other entries in list order and c the protected
 * count so far, slot i takes P's head when c < m[i] and P is not empty, else the smaller of the two
 * heads, else the head of the queue that is not empty (fair.py:231-245).  No float arithmetic, no
 * atomics: a row has the same result alone and in any batch.  Bad arguments (null pointers,
 * n_out > n_table, n_table > LK_FAIR_MAX_N) are LK_E_INVALID.
 * lk_fair_max_n: LK_FAIR_MAX_N as the library was built.
 * ---------------------------------------------------------------------- */
#define LK_FAIR_MAX_N 1024
int32_t lk_fair_max_n(void);
int lk_fair_rerank(const int32_t *d_lists, int64_t n_rows, int64_t row_len, int64_t ld,
                   const int32_t *d_lengths, const float *d_scores,
                   const uint8_t *d_is_protected, int64_t n_items, const int32_t *d_m_table,
                   int32_t n_table, int32_t n_out, int32_t *d_out_items, float *d_out_scores,
                   int32_t *d_out_pos, void *stream);

/* ------------------------------------------------------------------------
 * Randomized truncated SVD (csrc/svd.hip): the device steps of `BiasedSVDScorer.train`
 * (src/lenskit/sklearn/svd.py:74-104), which in the reference is sklearn's
 * `TruncatedSVD.fit_transform` -> `randomized_svd` -> `randomized_range_finder`.
 *
 * lk_csr_spmm replaces the products `A @ Q` / `A.T @ Q` of `randomized_range_finder`, `Q.T @ M` of
 * `randomized_svd` and `safe_sparse_dot(X, components_.T)` of `fit_transform`:
 *   d_out[r][c] = sum over the entries e of CSR row r of d_values[e] * d_x[d_indices[e]][c], c < l;
 *   d_x [n_cols x ld_x] and d_out [n_rows x ld_out] are padded float32 panels (leading dimensions
 *   multiples of 4 covering l rounded up to 4, ld_out <= 1024, bases 16-byte aligned); the columns
 *   [l, ld_out) of d_out are written as zero.  An index outside 0..n_cols-1 contributes nothing.
 *   A row of at most lk_spmm_split() entries is one fused-multiply-add chain per column in entry
 *   order; a longer one is cut into segments of that length, each such a chain, added in segment
 *   order.  No atomics: a row has the same bits alone, in any matrix, on any grid.  A^T Y is the
 *   same call on the transposed CSR (lk_csr_transpose, once per fit).
 *
 * lk_chol_upper_inverse replaces the normaliser between the products (sklearn: LU in the power
 * iterations, QR at the end; here CholeskyQR2 -- the result depends on the sketch's range only):
 *   d_gram [l x ld_gram] is the symmetric positive definite Gramian of a panel (lk_gramian; the
 *   lower triangle is read), G = R^T R with R upper triangular.  d_inverse [ld_out x ld_out]
 *   receives (R^-1)^T and d_lower (may be NULL) R^T, both lower triangular with zeros everywhere
 *   else -- as they stand the "items" operands of lk_score_dense for Y R^-1 with zero pad columns.
 *   One workgroup, the matrix in LDS as float32, the sums behind each entry carried in float64
 *   and rounded once: l <= lk_chol_max_l() = 192 (beyond that the caller uses the
 *   library's Cholesky and triangular solve).  A pivot that is not above 4 ulp of its diagonal
 *   entry (not positive to working precision: the panel has lost rank) stores `step` (!= 0) into
 *   *d_flag if that is still 0 and is replaced by the diagonal entry, so the outputs stay finite;
 *   the caller reads the flag once, when the whole factorisation is queued (as
 *   lk_als_check_status does), never between steps.
 * ---------------------------------------------------------------------- */
int32_t lk_spmm_split(void);
int lk_csr_spmm(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                const float *d_values, int64_t n_rows, int64_t n_cols, int64_t nnz,
                const float *d_x, int32_t ld_x, int32_t l, float *d_out, int32_t ld_out,
                void *stream);
int32_t lk_chol_max_l(void);
int lk_chol_upper_inverse(const float *d_gram, int32_t ld_gram, int32_t l, float *d_lower,
                          float *d_inverse, int32_t ld_out, int32_t *d_flag, int32_t step,
                          void *stream);

/* ------------------------------------------------------------------------
 * LightGCN (csrc/lightgcn.hip): the training step of `lenskit.graphs.lightgcn.LightGCNScorer`
 * (src/lenskit/graphs/lightgcn.py:108-324), whose arithmetic the reference tree states in
 * `FlexMFModel.update_convolution` / `forward` (src/lenskit/flexmf/_model.py:122-198) and
 * `FlexMFImplicitTrainer.prepare_data` / `train_batch` (_implicit.py:179-274).  n = items + users
 * nodes, items first; M is the symmetric n x n adjacency in CSR (int64 offsets, int32 columns, no
 * values), d_scale [n] = degree^-1/2 (0 for a node without entries), Mhat = diag(d) M diag(d).
 * Panels are float32 [n x ld], ld a multiple of 4 covering k <= LK_FLEXMF_MAX_K, bases 16-byte
 * aligned, pad columns zero.  Every call is asynchronous on `stream`; nothing is atomic on floats
 * and every sum has a fixed order.
 *
 * lk_lgcn_propagate replaces one `torch.mm(ui_mat, imat)` / `torch.mm(iu_mat, umat)` pair of
 * `update_convolution` (_model.py:134-140) together with the layer blend of `forward`
 * (_model.py:174-186), and the same products of autograd's backward pass:
 *   d_out[r] = a d_x[r] + (b d_scale[r]) sum over the entries e of row r of d_scale[col_e] d_t[col_e];
 *   d_x = NULL: no a d_x term.  A row of at most lk_spmm_split() entries is one
 *   fused-multiply-add chain per column in entry order from zero; a longer one is cut into
 *   segments of that length, each such a chain, added in segment order from zero; the row's scale
 *   is applied to the sum once and the a d_x term joins by one fused multiply-add.  A row has the
 *   same bits alone, in any matrix, on any grid.  An index outside 0..n-1 contributes nothing; a
 *   row without entries gives a d_x[r] (0 without d_x).  d_out must not alias d_x or d_t.
 *
 * lk_lgcn_pair_grad replaces `model(edges, mb_edges)`'s inner products, `batch_loss` and the
 * part of `loss.backward()` up to the propagated embeddings (lightgcn.py:289-292; the losses as
 * _implicit.py:399-409 states them, one negative per positive):
 *   s+ = xbar[u] . xbar[i+], s- = xbar[u] . xbar[i-] per sample (d_users, d_pos, d_neg: node
 *   numbers, duplicates allowed; a sample naming a node outside 0..n-1 takes no part);
 *   LK_FLEXMF_PAIRWISE  mean -log sigmoid(s+ - s-);
 *   LK_FLEXMF_LOGISTIC  (sum -log sigmoid(s+) + sum -log sigmoid(-s-)) / (2 batch);
 *   *d_loss receives the loss, *d_loss_sum (may be NULL) has it added; d_grad [n x ld] receives
 *   dloss/dxbar as a dense panel: zero, plus per node the sum of its samples' contributions in
 *   sample order (stable radix sort by node, then one wave per touched node, float64 sums
 *   rounded once), as lk_flexmf_step sums its rows.
 *
 * lk_adamw_dense replaces `optimizer.step()` of torch.optim.AdamW on one dense parameter
 * (lightgcn.py:239-249,293): every element of the k columns of d_param, d_exp_avg, d_exp_avg_sq
 * is updated from d_grad with the moments and the rounding of lk_flexmf_step's AdamW pass;
 * weight_decay = 0 is torch.optim.Adam.  bias_corr = 1 - beta^t of the step about to be taken.
 * Pad columns are left as they are.
 * ---------------------------------------------------------------------- */
int lk_lgcn_propagate(const int64_t *d_indptr, const int32_t *d_indices, const float *d_scale,
                      int64_t n, int64_t nnz, float a, const float *d_x, float b,
                      const float *d_t, int32_t k, int32_t ld, float *d_out, void *stream);
size_t lk_lgcn_pair_grad_workspace_bytes(int64_t batch);
int lk_lgcn_pair_grad(const float *d_xbar, int64_t n, int32_t k, int32_t ld, int32_t loss,
                      const int32_t *d_users, const int32_t *d_pos, const int32_t *d_neg,
                      int64_t batch, void *d_ws, float *d_grad, float *d_loss, float *d_loss_sum,
                      void *stream);
int lk_adamw_dense(float *d_param, float *d_exp_avg, float *d_exp_avg_sq, const float *d_grad,
                   int64_t n, int32_t k, int32_t ld, double lr, double weight_decay, double beta1,
                   double beta2, double eps, double bias_corr1, double bias_corr2, void *stream);

/* ------------------------------------------------------------------------
 * Hierarchical Poisson factorization (csrc/hpf.hip): the device steps of `HPFScorer.train`
 * (src/lenskit/hpf.py:81-100), which in the reference is `hpfrec.HPF.fit`.  The algorithm is
 * coordinate-ascent variational inference (Gopalan, Hofman, Blei 2015, Algorithm 1) on Gamma
 * shape / rate panels: gamma (users), lambda (items), kappa and tau (the hyper-rates).
 * Panels are float32 [n x ld], ld a multiple of 4 covering k <= LK_FLEXMF_MAX_K and at most
 * LK_FLEXMF_MAX_K, bases 16-byte aligned.  Every call is asynchronous on `stream`; nothing is
 * atomic on floats and every sum has a fixed order.
 *
 * lk_hpf_expect_log (hpf.py:81-100; Algorithm 1's E[log theta], E[log beta]):
 *   d_out[r][c] = psi(d_shp[r][c]) - log(d_rte[r][c]) for c < k, evaluated in float64 (digamma by
 *   its recurrence up to x >= 6, then the asymptotic series) and rounded to float32 once; the
 *   columns [k, ld) are written as zero.
 *
 * lk_hpf_shape_pass (hpf.py:81-100; Algorithm 1's multinomial phi and the shape updates): for
 *   every entry e = (r, col_e, y_e) of the CSR matrix, s_c = d_e_rows[r][c] + d_e_cols[col_e][c],
 *   m = max_c s_c, p_c = exp(s_c - m), Z = sum_c p_c (the lane's four columns in column order,
 *   then a butterfly over the row's lanes: an order that depends on ld alone), w = y_e / Z;
 *   d_out[r][c] = prior + sum_e w p_c, c < k; the columns [k, ld) are written as zero.  A row of
 *   at most lk_spmm_split() entries is one fused-multiply-add chain per column in entry order
 *   from zero; a longer one is cut into segments of that length, each such a chain, added in
 *   segment order from zero; the prior is added last.  A row has the same bits alone, in any
 *   matrix, on any grid.  An index outside 0..n_cols-1 contributes nothing; offsets that do not
 *   describe entries of the matrix make the row empty (d_out[r][c] = prior).  A spread of s
 *   beyond float32's exp range gives zero weights, never NaN.  The item side is the same call on
 *   the transposed CSR (lk_csr_transpose, once per fit) with the two E panels exchanged.
 *   d_out must not alias an operand.
 *
 * lk_hpf_rates (hpf.py:81-100; Algorithm 1's rate updates of one side and of its hyper-rate):
 *   d_rte[r][c] = shp_hyper / d_hyper_rte[r] + d_other_colsum[c], d_mean[r][c] = d_shp[r][c] /
 *   d_rte[r][c] (float32; pad columns zero), then d_hyper_rte[r] = prior_ratio + sum_c
 *   d_mean[r][c] (float64 in column order, rounded once) and d_colsum[c] = sum_r d_mean[r][c]:
 *   float64 partial sums over blocks of lk_hpf_rates_block() consecutive rows, each in row
 *   order, added in block order and rounded once -- a function of the panel alone.  d_ws:
 *   lk_hpf_rates_workspace_bytes(n, k) bytes.  d_colsum must not alias d_other_colsum.
 *
 * lk_hpf_loglik_rows (hpf.py:81-100; the data term of hpfrec's `train-llk` stopping criterion):
 *   d_out[r] = sum over the entries of row r of y_e log(d_theta[r] . d_beta[col_e]), the inner
 *   product and the sum in float64, the sum in entry order; an index outside 0..n_cols-1
 *   contributes nothing.
 * ---------------------------------------------------------------------- */
int lk_hpf_expect_log(const float *d_shp, const float *d_rte, int64_t n, int32_t k, int32_t ld,
                      float *d_out, void *stream);
int lk_hpf_shape_pass(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                      const float *d_values, int64_t n_rows, int64_t n_cols, int64_t nnz,
                      const float *d_e_rows, const float *d_e_cols, int32_t k, int32_t ld,
                      float prior, float *d_out, void *stream);
int32_t lk_hpf_rates_block(void);
size_t lk_hpf_rates_workspace_bytes(int64_t n, int32_t k);
int lk_hpf_rates(const float *d_shp, int64_t n, int32_t k, int32_t ld, double shp_hyper,
                 double prior_ratio, float *d_hyper_rte, const float *d_other_colsum,
                 float *d_rte, float *d_mean, float *d_colsum, void *d_ws, void *stream);
int lk_hpf_loglik_rows(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                       const float *d_values, int64_t n_rows, int64_t n_cols, int64_t nnz,
                       const float *d_theta, const float *d_beta, int32_t k, int32_t ld,
                       double *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Non-negative matrix factorization (csrc/nmf.hip): the coordinate sweep of `NMFScorer.train`
 * (src/lenskit/sklearn/nmf.py:72-110), which in the reference is sklearn's
 * `non_negative_factorization` -> `_fit_coordinate_descent` -> `_update_cdnmf_fast`.  One
 * half-iteration is lk_gramian (`HHt = Ht^T Ht + l2_reg I`), lk_csr_spmm (`XHt = X Ht`) and
 *
 * lk_nmf_cd_sweep: d_w [n x ld] (updated in place) and d_xht [n x ld] are padded float32 panels,
 *   ld = lk_padded_dim(k), 1 <= k <= lk_nmf_max_k() = 128; d_hht is [k x k] with leading dimension
 *   ld_hht.  With x = d_xht - l1_reg (rounded once), for every row i and t = 0 .. k-1 in order:
 *     grad = -x[i][t];  grad += d_hht[t][r] * d_w[i][r] for r = 0 .. k-1, product and sum rounded
 *     separately (no fused multiply-add, no tree; the division is IEEE);
 *     pg = d_w[i][t] == 0 ? min(0, grad) : grad;
 *     d_w[i][t] = max(d_w[i][t] - grad / d_hht[t][t], 0) unless d_hht[t][t] == 0.
 *   The rows are independent, so d_w has the bits of sklearn's float32 loop.  The pad columns of
 *   d_w are written as zero.  *d_violation (float64, device) receives the sum of |pg| over all
 *   rows and coordinates: float64 sums in a fixed order (coordinate order in a row, row order in a
 *   block of 64 rows, then the blocks), no floating-point atomics -- a function of the operands
 *   alone, but not sklearn's sequential float32 sum.  d_ws: lk_nmf_workspace_bytes(n) bytes.
 *   Asynchronous on `stream`.
 * ---------------------------------------------------------------------- */
int32_t lk_nmf_max_k(void);
size_t lk_nmf_workspace_bytes(int64_t n);
int lk_nmf_cd_sweep(float *d_w, int64_t n, int32_t k, int32_t ld, const float *d_hht,
                    int32_t ld_hht, const float *d_xht, float l1_reg, double *d_violation,
                    void *d_ws, void *stream);

/* ------------------------------------------------------------------------
 * FunkSVD (csrc/funksvd.hip): the featurewise SGD of `FunkSVDScorer.train`
 * (src/lenskit/funksvd.py:111-197) run level by level.  A sample reads and writes only its
 * user's and its item's entry of the feature's two columns, so with
 *   level(s) = 1 + max(level of the previous sample of u, level of the previous sample of i)
 * the samples of one level commute exactly and the levels in order give the bits of the
 * reference's sequential walk.
 *
 * lk_funksvd_plan_levels (HOST arrays; replaces nothing of the reference, which has no schedule):
 *   users / items [n] are the shuffled samples (funksvd.py:132-137), 0 <= users < n_users, 0 <=
 *   items < n_items (LK_E_INVALID otherwise).  level[n] receives each sample's level counted from
 *   0, *depth the number of levels.  One sequential O(n) pass.
 * lk_funksvd_plan_order (HOST arrays): the stable counting sort by level.  order[n]: sample
 *   positions in level order, ascending inside a level; level_ptr[depth + 1]: the levels' offsets
 *   in `order`; run_end[depth]: for a level inside a NARROW RUN -- a run of consecutive levels of
 *   at most lk_funksvd_narrow_width() = 64 samples each, extended level by level while it holds
 *   at most lk_funksvd_stage_samples() = 2048 samples, which the kernel stages in LDS -- one
 *   past the run's last level, for a wider level the level itself.
 *
 * lk_funksvd_train_feature: `epochs` calls of `FunkSVDTrainer::feature_epoch`
 *   (src/accel/funksvd.rs:67-128) for one feature, in ONE launch of one workgroup.  d_users,
 *   d_items, d_ratings, d_est [n] are the samples IN LEVEL ORDER (n = d_level_ptr[depth]),
 *   d_level_ptr / d_run_end the plan's arrays on the device, d_ucol [n_users] / d_icol [n_items]
 *   the feature's columns (updated in place).  Per sample, funksvd.rs:98-124 operation for
 *   operation in float64 with no fused multiply-add:
 *     pred = clamp((est + ufv * ifv) + trail, rmin, rmax);  err = r - pred;
 *     ufd = (err * ifv - reg * ufv) * lr;  ifd = (err * ufv - reg * ifv) * lr  (old ufv, ifv);
 *     ucol[u] = (float)(ufv + ufd);  icol[i] = (float)(ifv + ifd).
 *   rmin / rmax are -inf / +inf without a range.  d_sse[e] (float64) receives epoch e's sum of
 *   err^2: per-lane partial sums through a fixed tree -- repeatable, but not the reference's
 *   sequential sum (which is only logged, funksvd.rs:115,126).  With `finish` != 0 the launch
 *   ends with funksvd.py:188-190 in float32, product and sum rounded separately:
 *     est = clip(est + ucol[u] * icol[i], (float)rmin, (float)rmax).
 *   The columns sit in LDS when (n_users + n_items) * 4 <= lk_funksvd_lds_column_bytes(), in
 *   global memory otherwise or with LK_FUNKSVD_GLOBAL_COLUMNS in `flags` (same bits).  With the
 *   columns in LDS one wave walks a narrow run alone, fences between its levels; every other
 *   level, and every level with the columns in global memory, ends in a block barrier.  A call
 *   with e1 epochs followed by one with e2 gives the bits of one call with e1 + e2.
 *   Asynchronous on `stream`.
 * ---------------------------------------------------------------------- */
#define LK_FUNKSVD_GLOBAL_COLUMNS 1
int32_t lk_funksvd_narrow_width(void);
int32_t lk_funksvd_stage_samples(void);
size_t lk_funksvd_lds_column_bytes(void);
int lk_funksvd_plan_levels(const int32_t *users, const int32_t *items, int64_t n, int64_t n_users,
                           int64_t n_items, int32_t *level, int32_t *depth);
int lk_funksvd_plan_order(const int32_t *level, int64_t n, int32_t depth, int64_t *order,
                          int64_t *level_ptr, int32_t *run_end);
int lk_funksvd_train_feature(const int32_t *d_users, const int32_t *d_items,
                             const float *d_ratings, float *d_est, const int64_t *d_level_ptr,
                             const int32_t *d_run_end, int32_t depth, float *d_ucol,
                             float *d_icol, int64_t n_users, int64_t n_items, int32_t epochs,
                             int32_t finish, double lr, double reg, double trail, double rmin,
                             double rmax, int32_t flags, double *d_sse, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LKAMD_H */
