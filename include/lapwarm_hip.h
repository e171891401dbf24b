/*
 * lapwarm_hip.h -- C ABI of liblapwarm_hip.so, the MI355X (gfx950) implementation of the
 * warm-started LAP hot path.  Plain pointers and sizes only; no torch / C++ types.
 *
 * Two families of entry points:
 *   (1) drop-in replacements for the reference's native functions: HOST pointers, same
 *       argument meaning and return codes, one instance per call;
 *   (2) the batched DEVICE-pointer API that the pipeline and bench use: inputs already in
 *       HBM, stream-ordered, no host synchronisation inside (graph-capturable).
 *
 * Citations are relative to the reference repository root.
 */
#ifndef LAPWARM_HIP_H
#define LAPWARM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * (1) Drop-in, host pointers
 * ---------------------------------------------------------------------------------------- */

/* Replaces `lapjv_seeded` of LAP/lap/lapjv_seeded.h:8-13 (defined in
 * LAP/_lapjv_cpp/lapjv_seeded.cpp:19-173).  Identical signature and return codes:
 * 0 ok, -1 allocation failure, -2 n <= 0, -4 non-square, -3 infeasible after projection.
 * C, u_seed, v_seed are borrowed and never modified; x, y (caller-allocated, n each) are
 * written only when 0 is returned.  Other negative values: -5 n too large for this build
 * (> 16384), <= -100 internal guard tripped, <= -1000 HIP runtime error (-1000 - hipError_t). */
int lapjv_seeded(const double *C, int n_rows, int n_cols, long long *x, long long *y,
                 const double *u_seed, const double *v_seed, double eps);

/* Replaces `lapjv_internal(n, cost[], x, y)` of LAP/_lapjv_cpp/lapjv.cpp:323-346 (declared
 * LAP/_lapjv_cpp/lapjv.h:60-62) for a contiguous row-major matrix (the reference builds the
 * row-pointer array from exactly such a matrix, LAP/_lapjv_cpp/_lapjv.pyx:97-101).
 * Returns 0 or the codes above. */
int lapwarm_lapjv_dense(const double *C, int n, int *x, int *y);

/* gnn/features.py:161-243 `compute_row_features`: C (n*n fp64) -> feat (n*21 float32).
 * `topk16` (n*16 float32, ascending, +inf padded) may be NULL. */
int lapwarm_row_features(const double *C, int n, float *feat, float *topk16);

/* scripts/gnn_benchmark.py:262  v_j = min_i (C_ij - u_i), fp64 (u NULL -> plain column minima,
 * gnn/features.py:218). */
int lapwarm_min_trick(const double *C, int n, const double *u, double *v);

/* Row minima  out_i = min_j (C_ij - v_j)  (v NULL -> plain row minima): the `row_min` /
 * `u_cap` sweeps of solvers/seed_baselines.py:29 and solvers/advanced_dual.py:29. */
int lapwarm_row_min(const double *C, int n, const double *v, double *out);

/* solvers/advanced_dual.py:14-36 `project_feasible`: u, v updated in place. */
int lapwarm_project_feasible(const double *C, int n, double *u, double *v, int max_rounds, double tol);

/* solvers/advanced_dual.py:39-53 `reduce_costs`: out (n*n) = C - u 1^T - 1 v^T, shifted to be
 * non-negative when asked.  `min_out` (may be NULL) receives the unshifted minimum, which is what
 * `check_dual_feasible` (advanced_dual.py:56-63) tests. */
int lapwarm_reduce_costs(const double *C, int n, const double *u, const double *v, int shift_nonneg,
                         double *out, double *min_out);

/* solvers/dual_computation.py:13-74 `dual_from_matching_diff_constraints` for a full matching
 * (rows[k], cols[k]), k = 0..n-1, int32, in the caller's order; `tol` as the reference's.
 * Returns 0 with u, v (n each) written, or the per-instance codes of
 * lapwarm_oracle_duals_batched (1..5; u, v untouched), or -2 n <= 0, -5 n > 16384, -1 allocation
 * failure, <= -1000 HIP runtime error.  The reduced-cost matrix is lapwarm_reduce_costs(.., 0, ..). */
int lapwarm_oracle_duals(const double *C, int n, const int *rows, const int *cols, double *u, double *v,
                         double tol);

/* WarmStartLAPSolver.solve (solvers/warmstart_solver.py:31-63): C' = C - u 1^T - 1 v^T
 * (minus min(C') when negative and shift_nonneg), then the cold JV on C'.  One host-to-device
 * copy of C; the reduced matrix is formed and solved on the device; x, y [n] int32 come back. */
int lapwarm_warmstart_lapjv(const double *C, int n, const double *u, const double *v, int shift_nonneg,
                            int *x, int *y);

/* The reference's `lapjv(cost, extend_cost, cost_limit)` for a rectangular and / or cost-limited
 * problem (LAP/_lapjv_cpp/_lapjv.pyx:77-95 before the solve, :115-124 after it).  C (n_rows x n_cols,
 * row-major) is copied to the device as it is; the square matrix the reference solves is built there.
 * x [n_rows], y [n_cols] int32 with -1 for unmatched; *opt (may be NULL) = the sum of C[i][x[i]] over the
 * matched rows in numpy's summation order.  Returns 0, the codes of lapwarm_lapjv_extended_n, or those of
 * lapwarm_lapjv_dense; x, y, *opt are written only when 0 is returned. */
int lapwarm_lapjv_extended(const double *C, int n_rows, int n_cols, int extend_cost, double cost_limit,
                           int *x, int *y, double *opt);

/* n of the square problem the reference solves for this shape and these arguments (_lapjv.pyx:77-95):
 * n_rows + n_cols when cost_limit < inf, else max(n_rows, n_cols); -2 for n_rows or n_cols <= 0, -4 for a
 * non-square shape without extend_cost, -5 when n > 16384.  Needs no device. */
int lapwarm_lapjv_extended_n(int n_rows, int n_cols, int extend_cost, double cost_limit);

/* ------------------------------------------------------------------------------------------
 * (2) Batched, device pointers, stream-ordered.  `stream` is a hipStream_t (NULL = default).
 *     Every function returns 0 or <= -1000 (HIP error); per-instance codes go to `ret`.
 * ---------------------------------------------------------------------------------------- */

#define LAPWARM_STATS_PER_INSTANCE 32
/* stats[b][...]: 0 branch (1 ssp, 2 all matched, 3 fallback, 4 cold), 1 tight edges,
 * 2 free rows, 3 micro-ARR firings, 4 paths, 5 minima collections, 6 relax steps,
 * 7 relax elements (sum of n-hi), 8 path-init elements, 9 column-reduction elements,
 * 10 reduction-transfer rows, 11 ARR iterations, 12 internal error bits, 13 kernel time and
 * 14 greedy+micro-ARR time (10 ns ticks); 15 paths completed by the cooperative kernel | stop reason << 32
 * (-1: that kernel was not part of the solve); 16..26 its exchange-round counters; 27 row-reduction
 * iterations answered from candidate lists (cold solves); 16..31 cycle stamps in -DLAPWARM_STAMPS builds.
 * Where a solve consists of several launches (n >= 4428, cold solves with lists) slot 13 adds up the
 * preparation launch and the final one. */

size_t lapwarm_seeded_workspace_bytes(int batch, int n);
/* Workspace of the cold entry points below: the seeded workspace plus, from n = 512, the candidate lists
 * of the augmenting row reduction (1,544 bytes per row) and the hand-over state of the two launches a cold
 * solve then consists of (preparation with the lists, shortest augmenting paths; 44 bytes per row).  A
 * workspace of only lapwarm_seeded_workspace_bytes() is accepted too: one launch, every row-reduction
 * iteration scans its row (LAP/_lapjv_cpp/lapjv.cpp:76-149 as written). */
size_t lapwarm_lapjv_workspace_bytes(int batch, int n);

/* Batched lapjv_seeded over C[batch][n][n]; u_seed, v_seed [batch][n]; x, y [batch][n] int64;
 * ret [batch] int; stats [batch][32] int64 or NULL.  `threads_hint` = workgroup size of the
 * per-instance kernel (0 = auto). */
int lapwarm_seeded_batched(const double *C, int batch, int n, const double *u_seed,
                           const double *v_seed, double eps, long long *x, long long *y, int *ret,
                           long long *stats, void *workspace, size_t workspace_bytes,
                           int threads_hint, void *stream);

/* Batched cold lapjv; x, y [batch][n] int32.  Workspace: lapwarm_lapjv_workspace_bytes(). */
int lapwarm_lapjv_batched(const double *C, int batch, int n, int *x, int *y, int *ret,
                          long long *stats, void *workspace, size_t workspace_bytes,
                          int threads_hint, void *stream);

/* Batched rectangular / cost-limited lapjv, one shape per call.  C [batch][n_rows][n_cols]; x [batch][n_rows],
 * y [batch][n_cols] int32 with -1 for unmatched; opt [batch] fp64 (sum of C[i][x[i]] over the matched rows in
 * row order, numpy's pairwise summation of the compacted vector) and matched [batch] int (rows with
 * x != -1), either may be NULL; ret [batch]; stats [batch][32] or NULL: the cold solve's, for the n x n problem.
 * Instances with ret != 0: x, y all -1, opt NaN, matched 0.  Returns 0, the codes of
 * lapwarm_lapjv_extended_n (nothing is launched), -2 also for batch <= 0, batch > 65535 (the batch is one
 * dimension of the extension kernel's grid) or a workspace that is not 16-byte aligned (E is written with
 * 16-byte stores; C may have any 8-byte alignment), -1 workspace too small, <= -1000 HIP error.
 * Three steps on the caller's stream, kernels only: the extension kernel writes E [batch][n][n] into the
 * workspace (E[:n_rows, :n_cols] = C, cost_limit / 2. beside and below it, 0 in E[n_rows:, n_cols:]; zeros
 * around C without a limit; a square C without a limit is solved where it is), the cold solve of
 * lapwarm_lapjv_batched runs on E, the finish kernel maps x, y and sums opt.  The workspace holds E, the
 * solver's x, y [batch][n], the matched costs [batch][n_rows] and lapwarm_lapjv_workspace_bytes(batch, n);
 * every word of it that is read is written inside the call. */
size_t lapwarm_lapjv_extended_workspace_bytes(int batch, int n_rows, int n_cols, int extend_cost,
                                              double cost_limit);
int lapwarm_lapjv_extended_batched(const double *C, int batch, int n_rows, int n_cols, int extend_cost,
                                   double cost_limit, int *x, int *y, double *opt, int *matched, int *ret,
                                   long long *stats, void *workspace, size_t workspace_bytes,
                                   int threads_hint, void *stream);

/* As lapwarm_lapjv_batched, and also returns the optimal dual pair of each instance:
 * v [batch][n] = the solver's final column duals, u [batch][n] with u_i = C[i][x_i] - v[x_i]
 * (complementary slackness on the matched edges).  This is how the K2 configuration gets its
 * "oracle u" without the reference's O(n^3) Bellman-Ford (solvers/dual_computation.py:34-52). */
int lapwarm_lapjv_duals_batched(const double *C, int batch, int n, int *x, int *y, double *u, double *v,
                                int *ret, long long *stats, void *workspace, size_t workspace_bytes,
                                int threads_hint, void *stream);

/* The sweeps below restate NumPy expressions (np.min, np.minimum) and treat NaN as NumPy does: a NaN in C,
 * u or v makes every minimum it takes part in NaN (lapwarm_colmin_batched, lapwarm_rowmin_batched,
 * lapwarm_project_round_batched, gmin of lapwarm_reduce_costs_batched, and the host entries built on them).
 * The solver entry points keep the reference C++'s `<` comparisons, which pass over NaN. */
size_t lapwarm_sweep_workspace_bytes(int batch, int n);

/* out[b][j] = min_i (C[b][i][j] - u[b][i]); u may be NULL. */
int lapwarm_colmin_batched(const double *C, int batch, int n, const double *u, double *out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* out[b][i] = min_j (C[b][i][j] - v[b][j]); v may be NULL. */
int lapwarm_rowmin_batched(const double *C, int batch, int n, const double *v, double *out, void *stream);

/* feat [batch][n][21] float32, topk16 [batch][n][16] float32 or NULL; posenc [n][8] float32 is
 * the table of gnn/features.py:21-31 (built once per n on the host). */
int lapwarm_row_features_batched(const double *C, int batch, int n, const float *posenc, float *feat,
                                 float *topk16, void *workspace, size_t workspace_bytes, void *stream);

/* Ragged batches: `batch` square fp64 matrices of different sizes in one device buffer C.  offsets [batch]
 * int64 (device) is the element offset of instance b, a multiple of 8 bytes and no more; sizes [batch] int32
 * (device) is n_b; ld is the row stride in elements, 0 for n_b (packed, instances back to back), ld > 0 for a
 * common stride (the padded [batch][N][N] layout of `collate`, gnn/train_one_gnn.py:72-91, has ld = N and
 * offsets[b] = b N N).  N, 1..16384, is the padded width of every output; batch is 1..65535.  An instance with
 * sizes[b] outside 1..N (or above ld > 0) is treated as empty: padded outputs everywhere, ret[b] = 2, the code
 * of lapwarm_train_loss_forward.  Both entries return 0, -2 for N <= 0, batch outside 1..65535, ld < 0 or a
 * NULL pointer that may not be NULL, -5 for N > 16384, -1 workspace too small, <= -1000 HIP error.  Kernels
 * on the caller's stream only: no memset, allocation or host synchronisation, so a call can be captured into
 * a graph; every word of every output, and every workspace word that is read, is written inside the call. */
size_t lapwarm_ragged_workspace_bytes(int batch, int N);

/* out [batch][N]: out[b][j] = min_{i < n_b} (C_b[i][j] - u[b][i]) for j < n_b, 0 for j >= n_b; u [batch][N]
 * fp64 or NULL; NaN as np.min, like lapwarm_colmin_batched.  One kernel.  An instance whose base address and
 * row stride are multiples of 16 bytes is read with 16-byte loads, any other with 8-byte loads; the kernel
 * decides per instance.  The workspace is not used by this entry; its size is checked all the same. */
int lapwarm_colmin_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                          const double *u, double *out, void *workspace, size_t workspace_bytes, void *stream);

/* The row features, top-16, float32 costs and mask of a padded OneGNN batch in two kernels (column minima,
 * then one workgroup per padded row).  posenc [rows][8] float32 holds the tables of gnn/features.py:21-31 of
 * the distinct sizes, one after the other, and pos_off [batch] int32 (device) the first table row of instance
 * b.  feat [batch][N][21]: rows i < n_b are what lapwarm_row_features_batched gives for the n_b x n_b instance
 * alone, bit for bit; rows i >= n_b are 0.  topk16 [batch][N][16] or NULL: ascending, +inf beyond n_b and on
 * padded rows.  cost32 [batch][N][N] or NULL: (float)C on the prefix, 0 elsewhere, written while the row is
 * read for its features.  mask [batch][N] uint8 or NULL: 1 for i < n_b.  ret [batch]: 0 or 2. */
int lapwarm_row_features_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch,
                                int N, const float *posenc, const int *pos_off, float *feat, float *topk16,
                                float *cost32, unsigned char *mask, int *ret, void *workspace,
                                size_t workspace_bytes, void *stream);

/* lapjv_seeded of every instance of a ragged batch (C, offsets, sizes, ld, batch, N as above) in one call:
 * u_seed, v_seed [batch][N] fp64, read on the prefix of each instance only; x, y [batch][N] int64 with -1 beyond
 * n_b; ret [batch]; stats [batch][32] or NULL.  x, y, ret and stats of instance b are what
 * lapwarm_seeded_batched gives it alone (batch 1), the time slots 13, 14 and 16.. of stats apart: the
 * instance runs under the kernel instantiation it would get alone.  Instances whose solve plans have the same
 * kernel configuration (workgroup size, positions per lane, LDS level, register bound) share ONE launch, so
 * the call makes one prepare, two prelude, one projection launch and one solver launch per distinct
 * configuration -- at most seven -- whatever the number of distinct sizes.  host_sizes [batch] is a HOST copy
 * of sizes: the launches are planned from it and the stream is never synchronised (kernels only: the call
 * can be captured into a graph).  Every instance must be in the class whose plan is one launch with all
 * solver state in LDS and no helper workgroup: lapwarm_solver_uses_helpers(n_b) == 0, lapwarm_coop_members(n_b)
 * == 0 and n_b small enough for the state to fit LDS (with the default settings every n < 1024 and the odd n up to 3631).  A
 * launch takes the instances whose size ON THE DEVICE lies between the smallest and the largest host size of its
 * group, so an instance whose device size is not the host's is solved only if some launch of the call covers that
 * size (safely: the launch's threads and LDS hold for every n up to its largest); otherwise it stays as the prepare
 * step leaves it: x, y -1, ret 2, stats 0.  Returns 0, -2 (N <= 0, batch outside 1..65535, ld < 0, a NULL pointer other than stats, a host
 * size outside 1..N or above ld > 0), -5 (N > 16384), -6 (an instance outside the class: solve it with
 * lapwarm_seeded_batched), -1 (workspace too small), <= -1000 HIP error; only the last follows device work. */
size_t lapwarm_seeded_ragged_workspace_bytes(int batch, int N);
int lapwarm_seeded_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes, int ld,
                          int batch, int N, const double *u_seed, const double *v_seed, double eps, long long *x,
                          long long *y, int *ret, long long *stats, void *workspace, size_t workspace_bytes,
                          void *stream);
/* Host only, no device needed: group_of [batch] receives the launch of every instance of `sizes` (HOST,
 * [batch]), numbered from 0 in the order of first appearance; two instances share a launch exactly when their
 * solve plans have the same kernel configuration.  Returns the number of launches, -1 when an instance is
 * outside the class above, -2 for batch <= 0 or a NULL pointer. */
int lapwarm_seeded_ragged_groups(const int *sizes, int batch, int *group_of);

/* Cold lapjv of every instance of a ragged batch (C, offsets, sizes, host_sizes, ld, batch, N as for
 * lapwarm_seeded_ragged) in one call: x, y [batch][N] int64 with -1 beyond n_b; ret [batch]; stats [batch][32] or
 * NULL.  x, y, ret and the counters of instance b are what lapwarm_lapjv_batched gives it alone: the instance
 * runs under the kernel instantiation of its own cold plan, and instances whose cold plans have the same kernel
 * configuration share ONE launch (one init launch, then one solver launch per configuration).  Every instance
 * must be in the class whose cold plan is one launch with all solver state in LDS and no candidate lists: with
 * the default settings every n_b <= 511 (candidate lists start at 512; LAPWARM_ARR_LISTS=0 widens the class to
 * the sizes whose state fits LDS).  An instance whose size on the device lies in no launch of the call keeps
 * x, y -1, ret 2, stats 0.  Final duals are not returned: lapwarm_oracle_duals_ragged gives duals from a matching.
 * The workspace is not used; its size is checked all the same.  Kernels only, no host synchronisation: the
 * call can be captured into a graph.  Returns 0, -2 (N <= 0, batch outside 1..65535, ld < 0, a NULL pointer other
 * than stats, a host size outside 1..N or above ld > 0), -5 (N > 16384), -6 (an instance outside the class: solve
 * it with lapwarm_lapjv_batched), -1 (workspace too small), <= -1000 HIP error; only the last follows device work. */
size_t lapwarm_lapjv_ragged_workspace_bytes(int batch, int N);
int lapwarm_lapjv_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes, int ld,
                         int batch, int N, long long *x, long long *y, int *ret, long long *stats, void *workspace,
                         size_t workspace_bytes, void *stream);
/* Host only: as lapwarm_seeded_ragged_groups, for the cold plans and the class of lapwarm_lapjv_ragged. */
int lapwarm_lapjv_ragged_groups(const int *sizes, int batch, int *group_of);

/* lapwarm_lapjv_extended_batched for instances of different shapes and limits in one call.  Instance b is the
 * n_rows[b] x n_cols[b] fp64 matrix at C + offsets[b] (elements; 8-byte alignment is enough), rows ld elements
 * apart, or n_cols[b] when ld == 0 (packed), with its own cost_limit[b] (+inf: none); extend_cost is one flag
 * per call.  offsets, n_rows, n_cols, cost_limit are DEVICE arrays [batch]; host_rows, host_cols, host_limits
 * are HOST copies from which the call is planned (the stream is never synchronised and nothing is copied).
 * The extended size n_b is lapwarm_lapjv_extended_n's.  x [batch][R], y [batch][Q] int32 with -1 for unmatched
 * and beyond the instance's shape, R >= every n_rows, Q >= every n_cols; opt, matched [batch] or NULL; ret
 * [batch]; stats [batch][32] or NULL.  Everything of instance b is what lapwarm_lapjv_extended_batched gives it
 * alone (bit for bit; the time slots of stats apart).  Instances with ret != 0: x, y -1, opt NaN, matched 0.
 * Launches: one workgroup turns the device shapes into n_b and the offsets of the E_b; one launch (grid:
 * largest n x batch) writes every E_b [n_b][n_b], packed one behind the other in the workspace (sum of n_b^2
 * elements; a square instance without a limit is copied as well: one extra pass over a small matrix, where the
 * uniform entry solves it in place); one ragged cold solver launch per kernel configuration
 * (lapwarm_lapjv_ragged, every n_b must be in its class); one finish launch.  An instance whose shape on the
 * device is not what the host copies say is solved only if it still fits what was planned (R, Q, ld, the
 * largest n_b, the E area); otherwise it is treated as empty: x, y -1, opt NaN, matched 0, ret 2.
 * Every workspace word that is read is written inside the call.  Returns 0, -2 (batch outside 1..65535, a shape
 * with n_rows or n_cols <= 0, R or Q too small, ld < 0 or below an n_cols, a NULL pointer other than opt, matched
 * and stats, a workspace that is not 16-byte aligned), -4 (a non-square instance without extend_cost), -5 (an
 * n_b > 16384), -6 (an instance outside the class), -1 (workspace too small), <= -1000 HIP error; only the last
 * follows device work.  The workspace query returns 0 where the call would return -2, -4 or -5. */
size_t lapwarm_lapjv_extended_ragged_workspace_bytes(const int *host_rows, const int *host_cols,
                                                     const double *host_limits, int extend_cost, int batch);
int lapwarm_lapjv_extended_ragged(const double *C, const long long *offsets, const int *n_rows, const int *n_cols,
                                  const double *cost_limit, const int *host_rows, const int *host_cols,
                                  const double *host_limits, int ld, int extend_cost, int batch, int R, int Q, int *x,
                                  int *y, double *opt, int *matched, int *ret, long long *stats, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* Sparse LAPMOD (LAP/_lapjv_cpp/lapmod.cpp, lapmod_internal) of a batch of CSR problems of different n and nnz in
 * one call: one workgroup per instance.  cc (fp64) and kk (int32) hold the entries of all instances one behind the
 * other, instance b from nnz_offsets[b]; ii (int32) holds n_b + 1 row starts per instance from row_offsets[b],
 * counted from the instance's own first entry (ii[0] = 0).  nnz_offsets, row_offsets and sizes are DEVICE arrays
 * [batch]; host_sizes is the HOST copy the call is planned from.  fp_version: 1 find_path_sparse_1, 2
 * find_path_sparse_2, 3 chosen per matrix as the reference's FP_DYNAMIC does (nnz / n^2 > 0.25: 1).
 * x, y [batch][N] int32, -1 beyond n_b; v [batch][N] fp64 or NULL: the final column duals (NaN beyond n_b and where
 * ret != 0); ret [batch]; stats [batch][32] int64 or NULL: 0 free rows after column reduction and reduction transfer,
 * 1 and 2 after the first and second ARR pass (-1: not run), 3 ARR iterations, 4 paths, 5 find calls, 6 scan steps,
 * 7 the search that ran (0 none, 1, 2), 8 n, 9 nnz, 10 state in LDS (1) or in the workspace (0), 11 the search
 * fp_version selects for the matrix.  x, y and v of an instance with ret 0 are the reference's bit for bit.
 * ret: 0 solved; 1 no perfect matching (find_path_sparse_2 finds no candidate or scans a column that is absent from
 * its row, or the smallest d of a find_path_sparse_1 search is >= LARGE; the reference reads outside its arrays
 * there): x, y -1; 2 the instance is not what was planned or is malformed on the device (size outside 1..N, row
 * starts not ascending from 0, a row longer than n, a column outside 0..n-1, a cost outside [0, LARGE) or NaN):
 * x, y -1; < 0 a loop bound derived from n and nnz was exceeded.
 * Solver state lives in LDS for n_b <= lapwarm_lapmod_lds_max_n() (the largest n whose 48 n + 8 ceil(n / 32) bytes
 * fit 160 KB) and in the workspace above it.  lapwarm_lapmod_workspace_bytes: sizes and nnz are HOST arrays [batch]
 * (nnz may be NULL); 0 where the call would return -2 or -5.  Kernels only, no host synchronisation: the call can
 * be captured into a graph.  Returns 0, -2 (batch outside 1..65535, N <= 0, a host size outside 1..N, fp_version
 * outside 1..3, a NULL pointer other than v and stats, a workspace that is not 16-byte aligned), -5 (N or a host size > 65535: the reference's 32-bit `current * n` and n * n wrap from 65536 on),
 * -1 (workspace too small), <= -1000 HIP error; only the last follows device work. */
size_t lapwarm_lapmod_workspace_bytes(const int *sizes, const long long *nnz, int batch);
int lapwarm_lapmod_lds_max_n(void);
int lapwarm_lapmod_ragged(const double *cc, const int *kk, const int *ii, const long long *nnz_offsets,
                          const long long *row_offsets, const int *sizes, const int *host_sizes, int batch, int N,
                          int fp_version, int *x, int *y, double *v, int *ret, long long *stats, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Pruning and pricing of a ragged batch of dense cost matrices into CSR: the device steps of the exact dense solve
 * through lapwarm_lapmod_ragged ("Exact dense LAP through sparse LAPMOD").  C, offsets, sizes, ld, batch
 * and N as in the other ragged entries.  The round loop (grow, solve, price and grow, ... finish) lives in the
 * caller, which reads viol and ret back once per round: the loop is NOT graph-capturable; each entry here is kernels
 * on the caller's stream only, one grid over all instances each, without host synchronisation.
 *
 * lapwarm_prune_grow_ragged, one grow step.  key [batch][N] fp64 or NULL: key_ij = C_ij - key[b][j] (C_ij without).
 * x [batch][N] int32 or NULL: the bound of row i is C[i][x_i] - key[b][x_i] with x, +inf without (x needs key).
 * kk_in, ii_in, nnz_offsets_in, row_offsets_in: the current CSR in the layout of lapwarm_lapmod_ragged (columns
 * sorted and unique per row; it is the output of an earlier call), or all four NULL: every row holds its diagonal
 * only.  E_i is the set of columns absent from row i whose key is below the bound (fp64, as written).  The next
 * row holds the current columns and the min(m, |E_i|) members of E_i with the smallest key, ties to the lower
 * column, ascending in column; its values are read from C.  m in 1..256.  cc_out, kk_out, ii_out with
 * nnz_offsets_out, row_offsets_out and cap_out (DEVICE arrays [batch]; cap_out the entries instance b may write
 * from nnz_offsets_out[b]) receive the next CSR: ii_out holds n_b + 1 local row starts and the entries up to
 * ii_out[n_b] are written, the rest of the capacity is not touched; all six NULL: a pricing step that writes no
 * CSR.  added [batch] int64: entries of the next CSR minus those of the current one (of an absent one: 0), viol
 * [batch] int64: the sum of |E_i|, ret [batch] int32: 0; 3 the instance is not admissible (a cost outside [0, 1e6)
 * or NaN, a key that is not finite, an x_i or a current column outside 0..n_b-1, current row starts that do not
 * ascend), decided in the pass over C: no CSR entries are written; 4 the instance is treated as empty (size outside
 * 1..N or wider than ld > 0; lapwarm_rowmin_ragged reports 2 there, which is taken here by the caller's "not
 * certified"): no work; 5 the next CSR exceeds cap_out[b]: no CSR entries are written.  Three kernels (two for a
 * pricing step), two reads of C; nothing of size n x n is allocated; integer atomics in LDS only, so equal inputs
 * give equal bits.  Returns 0, -2 (N <= 0, batch outside 1..65535, ld < 0, m outside 1..256, x without key, a CSR
 * given in part, another NULL pointer), -5 (N > 16384), -1 (workspace below lapwarm_prune_workspace_bytes, which
 * is 0 out of range), <= -1000 HIP error; only the last follows device work.
 *
 * lapwarm_prune_finish_ragged: for the instances with ret[b] 0 or 2, u[b][i] = C[i][x_i] - v[b][x_i], cost[b] the
 * sum of C[i][x_i] taken serially in ascending i, and u, v set to 0 beyond n_b; for any other ret (and an instance
 * treated as empty or holding an x_i outside 0..n_b-1) u, v all 0 and cost inf.  x [batch][N] int32, v [batch][N]
 * fp64 in and out, ret [batch] in.  One kernel.  Returns 0, -2, -5 or <= -1000 as above. */
size_t lapwarm_prune_workspace_bytes(int batch, int N);
int lapwarm_prune_grow_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                              const double *key, const int *x, const int *kk_in, const int *ii_in,
                              const long long *nnz_offsets_in, const long long *row_offsets_in, int m, double *cc_out,
                              int *kk_out, int *ii_out, const long long *nnz_offsets_out,
                              const long long *row_offsets_out, const long long *cap_out, long long *added,
                              long long *viol, int *ret, void *workspace, size_t workspace_bytes, void *stream);
int lapwarm_prune_finish_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                const int *x, double *v, const int *ret, double *u, double *cost, void *stream);

/* One round of project_feasible: u = min(u, rowmin(C-v)); v = min(v, colmin(C-u));
 * gmin[b] = min((C-u)-v).  The host loop decides when to stop. */
int lapwarm_project_round_batched(const double *C, int batch, int n, double *u, double *v,
                                  double *gmin, void *workspace, size_t workspace_bytes, void *stream);

/* out [batch][n][n]; gmin [batch] receives the unshifted minima. */
int lapwarm_reduce_costs_batched(const double *C, int batch, int n, const double *u, const double *v,
                                 int shift_nonneg, double *out, double *gmin, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* Oracle duals (solvers/dual_computation.py:13-74 with tol = 1e-12), batched.  C [batch][n][n];
 * rows, cols [batch][n] int32 pairs in the caller's order; u, v [batch][n] fp64 (NaN where ret != 0);
 * ret [batch]: 0 ok, 1 negative cycle (the reference's RuntimeError), 2 dual infeasible after
 * reconstruction, 3 complementary slackness violated on a matched edge (its two AssertionErrors),
 * 4 the pairs are not a permutation, 5 C is not finite.  sweeps [batch][4] int32 or NULL:
 * Jacobi sweeps run (the last changed nothing), hop depth of the shortest-path tree, rows read by
 * the sweeps, 1 when the instance was replayed exactly.
 * Jacobi sweeps restricted to the rows whose source changed, double-buffered; instances that do not
 * settle within n - 1 sweeps, or whose predecessor graph has a cycle, replay the reference's
 * Gauss-Seidel loop exactly when n <= 2048; above 2048 such instances get ret 1 without a replay.
 * Sweeps are launched in chunks with one host synchronisation per chunk: NOT graph-capturable.
 * Workspace: lapwarm_oracle_duals_workspace_bytes(). */
size_t lapwarm_oracle_duals_workspace_bytes(int batch, int n);
int lapwarm_oracle_duals_batched(const double *C, int batch, int n, const int *rows, const int *cols, double *u,
                                 double *v, int *ret, int *sweeps, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* lapwarm_oracle_duals_batched of every instance of a ragged batch (C, offsets, sizes, ld, batch, N as above) in
 * one call.  rows, cols [batch][N] int32: the pairs of instance b, in the caller's order, on the prefix n_b.
 * u, v [batch][N] fp64: on the prefix what the uniform call writes (NaN for ret 1, 4 and 5), 0 beyond it.
 * ret [batch]: the codes of lapwarm_oracle_duals_batched, and 6 for an instance that is treated as empty (size
 * outside 1..N, or wider than ld > 0): it gets no work, u and v all 0, sweeps 0.  sweeps [batch][4] or NULL.
 * u, v, ret and sweeps of instance b are what lapwarm_oracle_duals_batched gives it alone (batch 1), bit for bit.
 * One init and one chain of sweep launches for all instances.  The chunk schedule is shared and runs to the
 * largest budget max_b (n_b - 1), taken from host_sizes [batch], a HOST copy of sizes (an entry the device would
 * treat as empty counts as 0); every instance keeps its own budget of n_b - 1 sweeps and its own check points on
 * the device.  As many host synchronisations as one uniform call of size max n_b: NOT graph-capturable.
 * An instance whose device size is larger than every host size makes only the sweeps of the host's budget; if it
 * has not settled by then, the last check hands it to the replay (n_b <= 2048: exact u, v and ret, with the
 * replayed counter set) or reports ret 1 (larger n_b).  Never a fault, and never ret 0 without duals.
 * Returns 0, -2 (N <= 0, batch outside 1..65535, ld < 0, a NULL pointer other than sweeps), -5 (N > 16384),
 * -1 (workspace too small), <= -1000 HIP error. */
size_t lapwarm_oracle_duals_ragged_workspace_bytes(int batch, int N);
int lapwarm_oracle_duals_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes,
                                int ld, int batch, int N, const int *rows, const int *cols, double *u, double *v,
                                int *ret, int *sweeps, void *workspace, size_t workspace_bytes, void *stream);

/* The dual utilities of solvers/advanced_dual.py:14-63 and the row minima of solvers/seed_baselines.py:29 for a
 * ragged batch (C, offsets, sizes, ld, batch, N as above; packed and padded layouts; the 16-byte load path is
 * chosen per instance as in lapwarm_colmin_ragged).  Every [batch][N] output is 0 beyond the prefix n_b.  An
 * instance that is treated as empty (size outside 1..N, or wider than ld > 0) gets no work: its outputs are 0
 * and ret[b] = 2; ret [batch] is 0 otherwise.  NaN as NumPy (np.min, np.minimum), like the uniform sweeps.  All
 * three entries return 0, -2 (N <= 0, batch outside 1..65535, ld < 0, a NULL pointer that may not be NULL), -5
 * (N > 16384), -1 (workspace below lapwarm_ragged_duals_workspace_bytes), <= -1000 HIP error.  Kernels on the
 * caller's stream only (each one grid over all instances, never a launch per instance or per size); every
 * word of every output, and every workspace word that is read, is written inside the call. */
size_t lapwarm_ragged_duals_workspace_bytes(int batch, int N);

/* out [batch][N]: out[b][i] = min_{j < n_b} (C_b[i][j] - v[b][j]) for i < n_b; v [batch][N] fp64 or NULL;
 * ret [batch] or NULL.  Row b is, bit for bit, what lapwarm_rowmin_batched gives instance b alone.  One kernel,
 * no host synchronisation: graph-capturable.  The workspace is not used; its size is checked all the same. */
int lapwarm_rowmin_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                          const double *v, double *out, int *ret, void *workspace, size_t workspace_bytes,
                          void *stream);

/* project_feasible (advanced_dual.py:14-36) of every instance: u, v [batch][N] fp64 in and out (read on the
 * prefix, 0 beyond it afterwards), gmin [batch] the last min((C - u) - v) of the instance, rounds [batch] int32
 * the rounds it ran, ret [batch].  An instance runs max(1, max_rounds) rounds at most and stops after the first
 * round with gmin >= -tol (a comparison NaN fails: an instance with NaN runs every round); the stop is per
 * instance and decided on the device, and the workgroups of a stopped instance return at once in later
 * rounds.  u, v and gmin of instance b are what lapwarm_project_feasible gives it alone, bit for bit.
 * A round is three kernels and two reads of C: rows (u), columns (v and the column's share of gmin, which is
 * cap_j - v_j with cap_j = min_i (C_ij - u_i): subtraction of v_j is monotone), and one workgroup per instance
 * that reduces gmin and sets the stop flag.  Rounds are launched in chunks of 1, 2, 4, ... 32 with one host
 * synchronisation after each chunk but the last, to learn whether any instance still runs: a call with
 * max_rounds <= 1 never synchronises, any other is NOT graph-capturable. */
int lapwarm_project_feasible_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch,
                                    int N, double *u, double *v, int max_rounds, double tol, double *gmin,
                                    int *rounds, int *ret, void *workspace, size_t workspace_bytes, void *stream);

/* reduce_costs (advanced_dual.py:39-53) of every instance: gmin [batch] receives the unshifted minima
 * min((C - u) - v); out, in the layout of C (same offsets and ld) or NULL, receives (C - u) - v on the prefix of
 * every instance, minus gmin[b] where shift_nonneg and gmin[b] < 0.  Elements of `out` outside the prefixes (the
 * padding of a padded layout, and all of an instance treated as empty, whose extent is unknown) are not
 * touched.  ret [batch] or NULL.  Bit for bit lapwarm_reduce_costs_batched per instance.  With out == NULL it
 * is the feasibility check (advanced_dual.py:56-63) and makes two kernels, else three; no host
 * synchronisation: graph-capturable. */
int lapwarm_reduce_costs_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                const double *u, const double *v, int shift_nonneg, double *out, double *gmin,
                                int *ret, void *workspace, size_t workspace_bytes, void *stream);

/* The synthetic cost families of the reference's dataset generator (data/generators.py, SYNTHETIC_FAMILIES), drawn
 * on the device straight into a ragged batch: C, offsets, sizes, ld, batch, N as above, C written instead of read.
 * Every value is a pure function of (seed, stream, element) under Philox4x32-10 with key (lo32(seed), hi32(seed))
 * and counter (lo32(group), hi32(group), stream, 0); csrc/cost_families.hpp states the draw rules, the streams and
 * the seven families (0 uniform, 1 metric, 2 low_rank, 3 clustered, 4 noisy_linear, 5 tie, 6 sparse).  An
 * instance's bits depend on its own (family, n, seed, params) only: not on the batch around it, its offset or ld.
 * family [batch] int32, seeds [batch] uint64, params [batch][4] fp64 = (rank | blocks | bins, sigma | noise | jitter
 * | sparsity, 0, 0), ret [batch] int32: all device arrays.  ret[b] = 0, 2 (size outside 1..N or wider than ld > 0:
 * no work) or 3 (family outside 0..6, or a rank outside 1..64 for low_rank and noisy_linear: nothing of the
 * instance is written).  Nothing outside the prefix [:n_b, :n_b] of an instance is written.  Three kernels on the
 * caller's stream, each one grid over all instances; no host synchronisation: graph-capturable.  No atomics: equal
 * arguments give equal bits.  Returns 0, -2 (N <= 0, batch outside 1..65535, ld < 0, a NULL pointer), -5
 * (N > 16384), -1 (workspace below lapwarm_cost_families_workspace_bytes, which is 0 out of range), <= -1000 HIP
 * error.
 * lapwarm_cost_family_draws: out[i], i < count, = U (kind 0, fp64), Z (kind 1, fp64) or I(., m) (kind 2, int32) of
 *   element first + i of stream stream_id, by the device functions the kernels use (out on the device; count < 2^39;
 *   kind outside 0..2, or kind 2 with m outside 1..2^31-1: -2). */
size_t lapwarm_cost_families_workspace_bytes(int batch, int N);
int lapwarm_generate_costs_ragged(double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                  const int *family, const unsigned long long *seeds, const double *params, int *ret,
                                  void *workspace, size_t workspace_bytes, void *stream);
int lapwarm_cost_family_draws(unsigned long long seed, unsigned int stream_id, int kind, unsigned long long first,
                              unsigned long long count, unsigned int m, void *out, void *stream);

/* The OneGNN training loss, gnn/train_one_gnn.py:180-226 `compute_loss` with its host greedy
 * `greedy_primal_upper` (:137-177), float32 terms and fp64 sums.  C [batch][n][n] float32, padded to the batch
 * maximum n; sizes [batch] int32 = n_b, the valid rows and columns of instance b are the prefix 0..n_b-1
 * (`collate`, :72-91); u_pred, u_target [batch][n].  Outputs: v_proj [batch][n] with v_j = min_i (C_ij - u_i)
 * (:189-193; 0 on padded columns); argmin_row [batch][n] int32, the row attaining v_j (-1 on padded columns);
 * assign [batch][n] int32, the greedy's column of row i (:143-152; -1 on padded rows); terms [batch][4] =
 * dual_lower (:195), feas (:197-201), u_reg (:212), primal_upper (:176), each an fp64 sum of the reference's
 * float32 terms rounded once; ret [batch]: 0, or 2 for sizes[b] outside 1..n (terms NaN, assign -1, v_proj 0).
 * Ties go to the lowest index (the row attaining a column minimum, the greedy's row order by min_j reduced_ij,
 * the column a row takes); the reference leaves them to np.argsort's unstable default (:145, :148).  A NaN in C
 * or u_pred reaches v_proj and feas as in torch.min / torch.relu; in the greedy a NaN reduced cost, of either
 * sign bit, ranks after +inf when a row chooses its column and is left out of the row minimum that orders the rows.
 * Returns 0, -2 for n <= 0, batch <= 0 or batch > 65535, -5 for n > 16384, -1 workspace too small,
 * <= -1000 HIP error.  Four kernels on the caller's stream, no host synchronisation; every workspace word
 * that is read is written inside the call.  The workspace keeps what the backward needs. */
size_t lapwarm_train_loss_workspace_bytes(int batch, int n);
int lapwarm_train_loss_forward(const float *C, int batch, int n, const int *sizes, const float *u_pred,
                               const float *u_target, float *v_proj, int *argmin_row, int *assign, float *terms,
                               int *ret, void *workspace, size_t workspace_bytes, void *stream);

/* Gradient of  w0 (primal_upper - dual_lower) + w1 feas + w2 u_reg  of every instance with respect to u_pred,
 * times grad_scale (1 / batch for the reference's batch means, :215-219; primal_upper is a constant, :176-177):
 *   grad_u[b][i] = grad_scale [ w0 (cnt_i - 1) + w1 (R_i - sum_{j: a_j = i} K_j) / n_b^2
 *                               + w2 2 (u_i - u_target_i) / n_b ]
 * with cnt_i = #{j: a_j = i}, R_i = #{j: h_ij > 0}, K_j = #{i: h_ij > 0}, h_ij = (u_i + v_j) - C_ij: what
 * autograd returns for :189-201 and :212 when no column minimum is tied.  Evaluated in fp64, rounded once;
 * 0 on padded rows and for instances with ret 2.  weights [3] float32 on the device (the reference: 1, 1, 0.1);
 * workspace: the one the forward call of the same batch, n, sizes, u_pred and u_target wrote; it is only read.
 * Returns as the forward. */
int lapwarm_train_loss_backward(int batch, int n, const int *sizes, const float *u_pred, const float *u_target,
                                const float *weights, float grad_scale, float *grad_u, const void *workspace,
                                size_t workspace_bytes, void *stream);

/* The DualGNN training loss, gnn/train.py:267-308 `compute_loss` (the same body in gnn/train_progressive.py:226-281)
 * with its host greedy (:224-264).  Everything is as in lapwarm_train_loss_forward but the third term: v_hint
 * [batch][n], the model's second output, takes the place of u_target, and terms [batch][4] = dual_lower (:282),
 * feas (:284-288), v_reg (:299), primal_upper (:295), with v_reg = sum_{j < n_b} (v_hint_j - v_proj_j)^2 / n_b: the
 * float32 difference and square of the reference, summed in fp64 in a fixed order and rounded once.  v_proj,
 * argmin_row, assign, ret, ties and NaN are bit for bit those of lapwarm_train_loss_forward on the same C, sizes and
 * u_pred.  The workspace (lapwarm_dual_loss_workspace_bytes: 0 out of range, else the training-loss workspace and,
 * behind it, d_j = v_hint_j - v_proj_j and S_i = sum_{j: a_j = i} d_j) keeps what the backward needs.  S_i is an
 * fp64 sum in ascending j, without floating-point atomics: equal inputs give equal bits.
 * Returns 0, -2 for n <= 0, batch <= 0 or batch > 65535, -5 for n > 16384, -1 workspace too small, <= -1000 HIP
 * error.  Four kernels on the caller's stream, no memset, no allocation, no host synchronisation; every workspace
 * word that is read is written inside the call. */
size_t lapwarm_dual_loss_workspace_bytes(int batch, int n);
int lapwarm_dual_loss_forward(const float *C, int batch, int n, const int *sizes, const float *u_pred,
                              const float *v_hint, float *v_proj, int *argmin_row, int *assign, float *terms,
                              int *ret, void *workspace, size_t workspace_bytes, void *stream);

/* Gradient of  w0 (primal_upper - dual_lower) + w1 feas + w2 v_reg  of every instance with respect to u_pred and
 * v_hint, times grad_scale (1 / batch for the reference's batch means, :301; primal_upper is a constant):
 *   grad_u[b][i]      = grad_scale [ w0 (cnt_i - 1) + w1 (R_i - sum_{j: a_j = i} K_j) / n_b^2 + w2 2 S_i / n_b ]
 *   grad_v_hint[b][j] = grad_scale   w2 2 d_j / n_b
 * with cnt, R, K as in lapwarm_train_loss_backward: v_j = C_{a_j j} - u_{a_j}, so v_reg reaches u_i through the
 * columns whose minimum row i attains.  Evaluated in fp64, rounded once; both 0 on the padding and for instances
 * with ret 2.  weights [3] float32 on the device (the reference: 1, 1, 0.1); workspace: the one the forward call of
 * the same batch, n, sizes, u_pred and v_hint wrote; it is only read.  One kernel; returns as the forward. */
int lapwarm_dual_loss_backward(int batch, int n, const int *sizes, const float *u_pred, const float *v_hint,
                               const float *weights, float grad_scale, float *grad_u, float *grad_v_hint,
                               const void *workspace, size_t workspace_bytes, void *stream);

/* OneGNN top-k refinement, aggregation part (gnn/one_gnn.py:139-155), float32:
 *   val_k = topk16[row][k] - u_pre[row]   (== topk(cost - u_pre): x -> x - c is monotone)
 *   w     = softmax(-val) over the finite entries (0 elsewhere)
 *   out[row][h] = sum_k w_k * GELU(w1[h] * val_k + b1[h]),  wsum[row] = sum_k w_k
 * The caller applies the second edge-MLP layer once per row: out @ W2^T + b2 * wsum (linearity).
 * topk16 [rows][16], u_pre [rows], w1/b1 [H], out [rows][H], wsum [rows]. */
int lapwarm_refine_aggregate_batched(const float *topk16, const float *u_pre, const float *w1,
                                     const float *b1, float *out, int rows, int H, int reserved,
                                     void *stream);
/* same call, with the [rows] weight sums; `wsum` may be NULL */
int lapwarm_refine_aggregate_wsum(const float *topk16, const float *u_pre, const float *w1,
                                  const float *b1, float *out, float *wsum, int rows, int H, void *stream);

/* Backward of lapwarm_refine_aggregate_wsum.  With G = grad_out [rows][H] = dL/dout and s = grad_wsum [rows] =
 * dL/dwsum (NULL: zero), x_kh = w1[h] val_k + b1[h] and GELU'(x) = Phi(x) + x phi(x):
 *   Q_k = sum_h G_h GELU(x_kh) + s,   D_k = sum_h G_h w1_h GELU'(x_kh)
 *   dval_k = w_k D_k - w_k (Q_k - sum_m w_m Q_m)   (0 where val_k is not finite)
 *   grad_u[row] = -sum_k dval_k
 *   grad_w1[h] = sum_row sum_k G_h w_k GELU'(x_kh) val_k,   grad_b1[h] = sum_row sum_k G_h w_k GELU'(x_kh)
 * topk16 is a constant: it has no gradient.  val, w and GELU are recomputed from the inputs; nothing of size
 * rows x 16 x H is stored.  float32 terms; the sums over rows are accumulated in fp64 in a fixed order (per
 * workgroup into the workspace, then by a second kernel) and rounded once, without atomics: equal inputs give
 * equal bits.  A row without a finite value gives grad_u == 0 and adds nothing to grad_w1 / grad_b1.
 * Two kernels on the caller's stream, no allocation, no host synchronisation; every workspace word that is read
 * is written inside the call.  Returns 0 (rows == 0: nothing is launched), -2 for rows < 0, H < 1, a NULL pointer
 * other than grad_wsum or ws_bytes below lapwarm_refine_backward_workspace_bytes(rows, H), <= -1000 HIP error. */
size_t lapwarm_refine_backward_workspace_bytes(int rows, int H);
int lapwarm_refine_backward(const float *topk16, const float *u_pre, const float *w1, const float *b1,
                            const float *grad_out, const float *grad_wsum, float *grad_u, float *grad_w1,
                            float *grad_b1, int rows, int H, void *ws, size_t ws_bytes, void *stream);

/* DualGNN graph features (the reference's compute_features, gnn/features.py:49-153) of a resident batch.
 *   edge_out [batch][n][n][10] f32: scaled cost, row rank, col rank, row gap, col gap, row tie, col tie, row entropy,
 *                                   col entropy, reduced cost C - u - min_i(C - u) (0 when u is NULL)
 *   row_out, col_out [batch][n][14] f32: min, max, mean, std, MAD, entropy, then posenc[i][0..8)
 * All statistics in fp64, rounded once.  Median and MAD are exact selections (a MAD below 1e-9 becomes 1e-9), the
 * entropy is the unstabilised exp(-C) form, the tie share counts gap <= 1e-3, ranks are STABLE (among equal values
 * the lower index ranks first) over n - 1 (0 at n = 1).  Column statistics are the row kernel on a transposed copy.
 * At every n a row's ranks come from a bitonic sort of (value, index) pairs in LDS, which also yields the median and
 * the MAD (a choice; counting ranks at small n has not been timed against it): n <= 4096, batch <= 32767.
 * Three kernels on the caller's stream, no allocation, no host synchronisation; every workspace word that is read
 * is written inside the call.  Returns 0, -1 (workspace too small), -2 (arguments), -5 (n > 4096), <= -1000 HIP. */
size_t lapwarm_graph_features_workspace_bytes(int batch, int n);
int lapwarm_graph_features_batched(const double *C, int batch, int n, const double *u_or_null, const float *posenc,
                                   float *edge_out, float *row_out, float *col_out, void *ws, size_t ws_bytes,
                                   void *stream);

/* DualGNN's DualLayer attention with the edge MLP's last Linear folded into the score weights (float32).
 * lapwarm_dual_edge_scores:  scores[b][dir][h][i][j] = G[dir * heads + h] . h2(i, j),
 *   h2 = GELU(W2 GELU(W1 f(i,j) + b1) + b2), f = edge_feat[b][i][j][0..10), erf GELU.
 *   W1 [128][10], b1 [128], W2 [128][128], b2 [128], G [2 * heads][128], scores [batch][2][heads][n][n];
 *   heads <= 8.  The three products run on the fp32 MFMA units (exact f32 fma chains).
 * lapwarm_dual_attention, both directions in one launch:
 *   row:  s_j = leaky_relu_0.2(a_row[b][h][i] + c_row[b][h][j] + scores[b][0][h][i][j] + kbias[0][h]), softmax over
 *         the j with mask[b][j] != 0, row_msg[b][i][h][:] = sum_j w_j col_val[b][j][h][:];
 *   col:  s_i = leaky_relu_0.2(a_col[b][h][j] + c_col[b][h][i] + scores[b][1][h][i][j] + kbias[1][h]), softmax over
 *         the unmasked i, col_msg[b][j][h][:] = sum_i w_i row_val[b][i][h][:].
 *   A masked query, or one without an unmasked key, gets a zero message.  mask [batch][n] bytes or NULL (all set);
 *   a_*, c_* [batch][heads][n]; values and messages [batch][n][heads * head_dim].  fp32 with max-subtraction, sums in
 *   a fixed order: equal inputs give equal bits.
 * lapwarm_dual_gnn_workspace_bytes is the size of the scores tensor, rounded up to 256 (0: arguments out of range).
 * Limits: batch <= 32767 and n <= 16384 for all three.  heads <= 8 for lapwarm_dual_edge_scores and the workspace
 *   query (2 * heads outputs fit one 16-wide MFMA tile).  lapwarm_dual_attention itself takes heads <= 65535 (the
 *   y dimension of its grid) and any head_dim >= 1, so it also serves scores that a caller produced elsewhere.
 * Returns 0, -2 (arguments, a heads value above the entry's limit included), -5 (n > 16384), <= -1000 HIP error. */
size_t lapwarm_dual_gnn_workspace_bytes(int batch, int n, int heads);
int lapwarm_dual_edge_scores(const float *edge_feat, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *G, float *scores, int batch, int n, int heads, void *stream);
int lapwarm_dual_attention(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                           const float *c_col, const float *kbias, const unsigned char *mask, const float *row_val,
                           const float *col_val, float *row_msg, float *col_msg, int batch, int n, int heads,
                           int head_dim, void *stream);

/* DualGNN on a batch of instances of different sizes (C, offsets, sizes, ld, batch, N as in lapwarm_colmin_ragged;
 * N <= 4096 and batch <= 32767 for the features, the limits of the uniform entries for the other two).
 * lapwarm_graph_features_ragged: lapwarm_graph_features_batched per instance, in the same three kernels, every
 *   output padded to N and written in full: edge_out [batch][N][N][10], row_out, col_out [batch][N][14] f32, mask
 *   [batch][N] bytes (1 on the prefix), ret [batch] (0; 2 for an instance treated as empty: all-zero outputs).  On the
 *   prefix of instance b the outputs are, bit for bit, what lapwarm_graph_features_batched gives the instance alone;
 *   outside it they are 0.  u [batch][N] fp64 is read on each prefix, or NULL (channel 9 is 0); posenc and pos_off
 *   as in lapwarm_row_features_ragged.  The workspace has the layout of the uniform call with n = N.
 * lapwarm_dual_edge_scores_ragged: lapwarm_dual_edge_scores with sizes [batch] on the device.  Only the edges
 *   (i, j < sizes[b]) are computed (a row's tail rounded up to 16 edges) and written; scores outside the prefixes
 *   are NOT written.  On the prefixes the bits are lapwarm_dual_edge_scores's on the same padded input.
 * lapwarm_dual_attention_ragged: lapwarm_dual_attention with the prefix [0, sizes[b]) as the mask.  Blocks of padded
 *   queries write zero messages and read nothing, the key loops stop at the prefix and no score outside a prefix is
 *   loaded (it may hold anything).  The messages are, bit for bit, those of lapwarm_dual_attention with that mask.
 * A size outside 1..N is an empty instance.  Returns 0, -1 (workspace too small), -2 (arguments), -5 (N above the
 * entry's limit), <= -1000 HIP error; argument codes come before any HIP call. */
size_t lapwarm_graph_features_ragged_workspace_bytes(int batch, int N);
int lapwarm_graph_features_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                  const double *u_or_null, const float *posenc, const int *pos_off, float *edge_out,
                                  float *row_out, float *col_out, unsigned char *mask, int *ret, void *ws,
                                  size_t ws_bytes, void *stream);
int lapwarm_dual_edge_scores_ragged(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                    const float *b2, const float *G, float *scores, const int *sizes, int batch, int n,
                                    int heads, void *stream);
int lapwarm_dual_attention_ragged(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                  const float *c_col, const float *kbias, const int *sizes, const float *row_val,
                                  const float *col_val, float *row_msg, float *col_msg, int batch, int n, int heads,
                                  int head_dim, void *stream);

/* DualGNN training: the backward of the two kernels above (float32, heads <= 8, batch and n as the forward).
 * lapwarm_dual_attention_stats / _stats_ragged: lapwarm_dual_attention / _ragged that also write, per query, the
 *   maximum of its leaky_relu scores and the sum of exp(s - max): row_stats, col_stats [batch][heads][n][2].  The
 *   messages are bit for bit those of the entries without statistics.
 * lapwarm_dual_attention_backward, per (b, direction, h), q the query and k the key, from dmsg = dL/dmsg:
 *     z[q,k] = ((a[q] + c[k]) + S[q,k]) + kb,  s = leaky_relu_0.2(z),  w[q,k] = exp(s - max_q) / sum_q
 *     delta[q] = dmsg[q] . msg[q],   dw[q,k] = dmsg[q] . val[k]
 *     dz[q,k]  = w[q,k] (dw[q,k] - delta[q]) (z >= 0 ? 1 : 0.2), exactly 0 where q or k is masked
 *     dS = dz (in the layout of the scores: [i][j] for both directions),  da[q] = sum_k dz,  dc[k] = sum_q dz,
 *     dkb[direction][h] = sum_{b,q,k} dz,   dval[k] = sum_q w[q,k] dmsg[q]
 *   The kernel forms delta[q] as sum_k w[q,k] dw[q,k], which is dmsg[q] . msg[q]: built from the numbers it is
 *   subtracted from, its rounding cancels in sum_k dz as in exact arithmetic (a query with one key gets exactly 0).
 *   (val is col_val for the row direction and row_val for the column direction, so d_col_val comes from the row
 *   direction.)  mask and sizes as in the forward, both nullable, sizes taking precedence.  With sizes no score and
 *   no dS entry outside a prefix is read or written; padded or masked queries and keys get exactly 0 in da, dc and
 *   dval.  Three kernels: a query-major pass over 16 queries (dS, da, one partial of dkb per workgroup), a key-major
 *   pass over 16 keys (dc from dS read back, dval with w recomputed), and the reduce of the partials in fp64.
 *   fp32 sums in a fixed order, no atomics: equal inputs give equal bits.
 * lapwarm_dual_edge_scores_backward, from dS [batch][2 * heads][n][n] and the forward's inputs, with
 *   x1 = W1 f + b1, h1 = GELU(x1), x2 = W2 h1 + b2, h2 = GELU(x2), GELU'(x) = Phi(x) + x phi(x), per edge e:
 *     dh2 = G^T dS_e,  dx2 = dh2 * GELU'(x2),  dh1 = W2^T dx2,  dx1 = dh1 * GELU'(x1)
 *     dG = sum_e dS_e h2^T,  dW2 = sum_e dx2 h1^T,  db2 = sum_e dx2,  dW1 = sum_e dx1 f^T,  db1 = sum_e dx1
 *   dW1 [128][10], db1 [128], dW2 [128][128], db2 [128], dG [2 * heads][128]; edge_feat has no gradient.  Nothing
 *   of width 128 per edge is kept from the forward: per chunk of lapwarm_dual_backward_chunk edges one kernel
 *   recomputes the edge MLP on the MFMA units and leaves h1, h2, dx2, dx1, dS and f as rows in the workspace, a
 *   second forms the five sums over a fixed slice of rows per workgroup on the same units, a third adds the
 *   workgroups and the chunks in fp64 in order and rounds once after the last chunk.  With sizes (nullable) only
 *   the edges (i, j < sizes[b]) are walked and dS outside the prefixes is never read.  Equal inputs give equal bits.
 * lapwarm_dual_backward_workspace_bytes: the workspace of either backward (the larger), at most 64 MiB of rows plus
 *   the partials; 0 for arguments out of range (the limits of lapwarm_dual_gnn_workspace_bytes).  Every workspace
 *   word that is read is written inside the call.
 * Returns 0, -1 (workspace too small), -2 (arguments), -5 (n > 16384), <= -1000 HIP error; argument codes come
 * before any HIP call. */
int lapwarm_dual_attention_stats(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                 const float *c_col, const float *kbias, const unsigned char *mask,
                                 const float *row_val, const float *col_val, float *row_msg, float *col_msg,
                                 float *row_stats, float *col_stats, int batch, int n, int heads, int head_dim,
                                 void *stream);
int lapwarm_dual_attention_stats_ragged(const float *scores, const float *a_row, const float *c_row,
                                        const float *a_col, const float *c_col, const float *kbias, const int *sizes,
                                        const float *row_val, const float *col_val, float *row_msg, float *col_msg,
                                        float *row_stats, float *col_stats, int batch, int n, int heads, int head_dim,
                                        void *stream);
size_t lapwarm_dual_backward_workspace_bytes(int batch, int n, int heads);
int lapwarm_dual_backward_chunk(void);
int lapwarm_dual_attention_backward(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                    const float *c_col, const float *kbias, const unsigned char *mask,
                                    const int *sizes, const float *row_val, const float *col_val,
                                    const float *row_msg, const float *col_msg, const float *row_stats,
                                    const float *col_stats, const float *d_row_msg, const float *d_col_msg, float *dS,
                                    float *da_row, float *dc_row, float *da_col, float *dc_col, float *dkb,
                                    float *d_row_val, float *d_col_val, int batch, int n, int heads, int head_dim,
                                    void *workspace, size_t workspace_bytes, void *stream);
int lapwarm_dual_edge_scores_backward(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                      const float *b2, const float *G, const float *dS, const int *sizes, float *dW1,
                                      float *db1, float *dW2, float *db2, float *dG, int batch, int n, int heads,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* DualGNN training with the reference's two dropouts inside the fused region: in the edge MLP after its first GELU and
 * on the attention weights.  No mask is stored; the backward regenerates the forward's.  The keep rule is a pure
 * function of (seed, stream, element index e), Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, key increments
 * 0x9E3779B9, 0xBB67AE85):
 *     key (lo32(seed), hi32(seed)),  counter (lo32(e >> 2), hi32(e >> 2), stream, 0),  word = output number e & 3;
 *     e is kept iff word >= T, T = floor(p 2^32) formed in double;  a kept value is multiplied by float(1 / (1 - p)).
 *   The logical tensors are indexed in the PADDED layout, so tiling, chunking and sizes cannot change a mask:
 *     stream 0, edge MLP:           e = ((b n + i) n + j) 128 + unit,  applied to h1 = GELU(W1 f + b1);
 *     stream 1, attention weights:  e = (((b 2 + dir) heads + h) n + q) n + k,  q the query and k the key of the
 *                                   direction (dir = 1: the query is the column j), applied to the softmax weights
 *                                   after the masked pairs are zeroed.
 * lapwarm_dual_edge_scores_dropout: lapwarm_dual_edge_scores (sizes NULL) or _ragged with h1 replaced by
 *   keep scale h1 before the second product.
 * lapwarm_dual_attention_stats_dropout: lapwarm_dual_attention_stats (mask nullable; sizes nullable, taking precedence)
 *   whose messages are sum_k w[q,k] keep scale val[k]; the statistics are those of the undropped softmax.
 * lapwarm_dual_attention_backward_dropout: lapwarm_dual_attention_backward with
 *     dw[q,k] = keep scale (dmsg[q] . val[k]),  delta[q] = sum_k w dw (= dmsg[q] . msg[q], msg the dropped message),
 *     dz = w (dw - delta) slope,  dval[k] = sum_q w keep scale dmsg[q].
 * lapwarm_dual_edge_scores_backward_dropout: lapwarm_dual_edge_scores_backward whose recompute applies the mask:
 *     h1 is the dropped one (in dW2 too) and dx1 = dh1 keep scale GELU'(x1).
 *   The four take the argument lists of the entries without dropout plus seed and p, the same seed and p in the forward
 *   and its backward.  p outside [0, 1) or NaN: -2 before any HIP call.  With p == 0 they give the bits of the entries
 *   without dropout.  No scratch, no atomics: equal inputs and an equal seed give equal bits.
 * lapwarm_dual_dropout_keep: keep[i] = 1 if element first + i of stream stream_id is kept, else 0, i < count, by the
 *   device function the kernels use (keep on the device; count < 2^39). */
int lapwarm_dual_edge_scores_dropout(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                     const float *b2, const float *G, float *scores, const int *sizes_or_null, int batch,
                                     int n, int heads, unsigned long long seed, double p, void *stream);
int lapwarm_dual_attention_stats_dropout(const float *scores, const float *a_row, const float *c_row,
                                         const float *a_col, const float *c_col, const float *kbias,
                                         const unsigned char *mask_or_null, const int *sizes_or_null,
                                         const float *row_val, const float *col_val, float *row_msg, float *col_msg,
                                         float *row_stats, float *col_stats, int batch, int n, int heads, int head_dim,
                                         unsigned long long seed, double p, void *stream);
int lapwarm_dual_attention_backward_dropout(const float *scores, const float *a_row, const float *c_row,
                                            const float *a_col, const float *c_col, const float *kbias,
                                            const unsigned char *mask, const int *sizes, const float *row_val,
                                            const float *col_val, const float *row_msg, const float *col_msg,
                                            const float *row_stats, const float *col_stats, const float *d_row_msg,
                                            const float *d_col_msg, float *dS, float *da_row, float *dc_row,
                                            float *da_col, float *dc_col, float *dkb, float *d_row_val,
                                            float *d_col_val, int batch, int n, int heads, int head_dim,
                                            void *workspace, size_t workspace_bytes, unsigned long long seed, double p,
                                            void *stream);
int lapwarm_dual_edge_scores_backward_dropout(const float *edge_feat, const float *W1, const float *b1,
                                              const float *W2, const float *b2, const float *G, const float *dS,
                                              const int *sizes, float *dW1, float *db1, float *dW2, float *db2,
                                              float *dG, int batch, int n, int heads, void *workspace,
                                              size_t workspace_bytes, unsigned long long seed, double p, void *stream);
int lapwarm_dual_dropout_keep(unsigned long long seed, unsigned int stream_id, unsigned long long first,
                              unsigned long long count, double p, unsigned char *keep, void *stream);

/* The edge MLP of DualGNN on the bf16 MFMA units (v_mfma_f32_16x16x32_bf16), forward and backward.  Conversions are
 * round-to-nearest-even from fp32 to bf16, at exactly these points: edge_feat when it is loaded; W1, W2 and G when they
 * are staged; h1 after GELU and dropout (keep scale gelu(x1)); h2 after GELU; in the backward dS, dh2pre = dh2 GELU'(x2),
 * dh1pre and the column of ones where they become MFMA operands.  b1, b2, both pre-activations, GELU, GELU', the scores
 * and the sums of the weight gradients (fp32 per workgroup slice, fp64 across slices and chunks, rounded once) are as
 * in the fp32 entries.  The backward recomputes h1 and h2 as the forward does and returns the gradient of the fp32
 * function at the rounded values (straight-through rounding).  No atomics: equal inputs and an equal seed give equal
 * bits; the dropout mask of a seed is the mask of the fp32 entries.
 * lapwarm_dual_edge_scores_bf16: the argument list of lapwarm_dual_edge_scores_dropout; sizes NULL for the uniform
 *   batch, p == 0 for no dropout.
 * lapwarm_dual_edge_scores_backward_bf16: the argument list of lapwarm_dual_edge_scores_backward_dropout with the seed
 *   and p of the forward; the workspace is lapwarm_dual_backward_workspace_bytes, unchanged. */
int lapwarm_dual_edge_scores_bf16(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                  const float *b2, const float *G, float *scores, const int *sizes_or_null, int batch,
                                  int n, int heads, unsigned long long seed, double p, void *stream);
int lapwarm_dual_edge_scores_backward_bf16(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                           const float *b2, const float *G, const float *dS, const int *sizes,
                                           float *dW1, float *db1, float *dW2, float *db2, float *dG, int batch, int n,
                                           int heads, void *workspace, size_t workspace_bytes, unsigned long long seed,
                                           double p, void *stream);

/* Profiling hook for bench.py: when enabled, lapwarm_seeded_batched / lapwarm_lapjv_batched /
 * lapwarm_seeded_ragged / lapwarm_lapjv_ragged / lapwarm_lapjv_extended_ragged bracket their solver launches
 * with HIP events on the caller's stream;
 * lapwarm_profile_last_solver_ms() waits for the last bracket and returns its duration. */
void lapwarm_profile_enable(int on);
double lapwarm_profile_last_solver_ms(void);

/* 1 when lapwarm_seeded_batched launches one helper workgroup per instance for this n (the helper
 * pulls announced head rows towards the L2 its solver shares; LAPWARM_HELPER=0 turns it off):
 * the solver kernel then occupies about 2 * batch CUs.  n = 1024 .. 8192. */
int lapwarm_solver_uses_helpers(int n);

/* Number of single-wave workgroups ("members", one compute unit each) that share ONE instance's
 * shortest-augmenting-path phase for this n, or 0 when that phase runs inside the one-workgroup-per-
 * instance kernel (n < 4428 by default; LAPWARM_COOP=0 / LAPWARM_COOP_MIN_N change it).  New, additive:
 * the reference has no counterpart (its _ca_dense, LAP/_lapjv_cpp/lapjv.cpp:286-319, is serial). */
int lapwarm_coop_members(int n);

/* Misc */
/* The text of the calling thread's last failure that has one: every -1 of an entry point that takes a workspace
 * ("workspace too small: <given> < <needed>", bytes), every -6 and every code <= -1000 (the HIP call and its
 * error string).  Argument codes (-2, -4, -5) leave it as it was. */
const char *lapwarm_last_error(void);
int lapwarm_device_count(void);
const char *lapwarm_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* LAPWARM_HIP_H */
