// jv_solver.hpp -- host-visible interface of the per-instance solver kernel (jv_solver.hip)
// and of the dense sweep kernels (dense_sweeps.hip).  Internal to the shared library; the
// public C ABI is include/lapwarm_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lapwarm {

constexpr int kModeSeeded = 0;  // continue from the dense prelude (lapjv_seeded)
constexpr int kModeCold = 1;    // plain lapjv

constexpr int kBranchSsp = 1;
constexpr int kBranchAllMatched = 2;
constexpr int kBranchFallback = 3;
constexpr int kBranchCold = 4;

constexpr int kStatsPerInstance = 32;
constexpr size_t kLdsBudgetBytes = 160 * 1024;

constexpr int kHandInts = 16;
constexpr int kCoopStats = 16;

// hand[]: the hand-over block of one instance, kHandInts ints: what jv_instance_kernel (phases 1, 2, 3) and
// coop_ssp_kernel tell each other between the launches of a solve that consists of several.  Phase 1
// writes every slot.
enum HandSlot {
    kHandFreeRows = 0,  // rows the shortest-path phase has to augment (0: nothing for it to do)
    kHandPathsDone,     // resume index into the free-row list: paths completed so far
    kHandCoopErr,       // error code of the cooperative kernel's leader
    kHandStopReason,    // why the cooperative kernel stopped before the last path (0: it did not)
    kHandMemberErr,     // error seen by a member other than the leader (atomicMax)
    // what phase 1 knows and phase 2 reports
    kHandBranch,
    kHandTightEdges,
    kHandFreeAfterGreedy,
    kHandArrFired,      // micro-ARR firings
    kHandTransferRows,  // reduction-transfer rows
    kHandArrIters,
    kHandColredLo,      // column-reduction elements, 64 bits in two slots
    kHandColredHi,
    kHandPrepErr,       // error of phase 1, or of a phase 3
    kHandListIters,     // row-reduction iterations answered from candidate lists
    kHandPrepTicks,     // duration of the phase-1 launch, 10 ns ticks (saturating)
};
static_assert(kHandPrepTicks == kHandInts - 1, "hand[] layout");

// coop_ssp_kernel: may it take the next path of this instance?
__host__ __device__ __forceinline__ bool hand_coop_may_run(const int *hand)
{
    return !(hand[kHandFreeRows] <= 0 || hand[kHandCoopErr] != 0 || hand[kHandMemberErr] != 0 ||
             hand[kHandStopReason] != 0 || hand[kHandPathsDone] >= hand[kHandFreeRows]);
}

// cstats[]: kCoopStats int64 per instance, zeroed by phase 1: what the shortest-path phase counts outside
// phase 2 (coop_ssp_kernel, and phase 3 for the paths it runs).
enum CoopStat {
    kCsPaths = 0,  // the path counters: phase 2 adds them to its own
    kCsFinds,
    kCsScanSteps,
    kCsScanElems,
    kCsInitElems,
    kCsReport,               // ---- the block phase 2 copies to stats[kStCoopReport ..] starts here
    kCsRounds = kCsReport,   // exchange rounds (low 40 bits) | all members on one XCD << 40
    kCsStamp0,               // 6 cycle-stamp sums (-DLAPWARM_COOP_STAMPS builds)
    kCsPollMax = kCsStamp0 + 6,  // stamp builds, over the members (atomicMax on the slot as unsigned):
    kCsWorkMax,                  //   largest poll / work total,
    kCsPollMinC,                 //   complement of the smallest poll total,
    kCsWorkMinC,                 //   ... and of the smallest work total
    kCsOutsidePaths = kCsWorkMinC,  // shipped builds: paths searched by phase 3, one launch each
    // (as before these names existed, a COOP_STAMPS build that runs a phase 3 adds that 1 to the complement
    // of the smallest work total: the two uses of the last slot were never separated)
};
constexpr int kCoopReportSlots = kCoopStats - kCsReport;
static_assert(kCsOutsidePaths == kCoopStats - 1, "cstats layout");

// stats[]: kStatsPerInstance int64 per instance.  The slot numbers are public ABI (include/lapwarm_hip.h
// documents them; Python indexes by number); these names are for the library's own code.
enum StatSlot {
    kStBranch = 0,
    kStTightEdges,
    kStFreeRows,
    kStArrFired,
    kStPaths,
    kStFinds,
    kStScanSteps,
    kStScanElems,
    kStInitElems,
    kStColredElems,
    kStTransferRows,
    kStArrIters,
    kStErr,
    kStKernelTicks,  // 10 ns ticks; a solve of several launches adds the preparation launch
    kStSerialTicks,  // greedy + micro-ARR part (SSP branch)
    kStCoopPaths,    // paths the cooperative kernel completed | why it stopped early << 32 (-1: not used)
    kStCoopReport,   // kCoopReportSlots slots: cstats[kCsReport ..]
    kStListIters = 27,          // row-reduction iterations answered from candidate lists
    kStStamps = kStCoopReport,  // -DLAPWARM_STAMPS builds: kStampSlots cycle stamps instead (they overwrite
                                // the cooperative report and kStListIters, as they always did)
};
constexpr int kStampSlots = 16;
static_assert(kStCoopReport == 16 && kStCoopReport + kCoopReportSlots <= kStListIters, "stats layout");
static_assert(kStStamps + kStampSlots == kStatsPerInstance, "stats layout");

struct SolverParams {
    const double *C;  // [batch][n][n] row-major fp64
    int n;
    int batch;
    int mode;
    // seeded mode inputs, produced by the prelude kernel
    const double *u_tight;       // [batch][n]      u after row tightening (P3)
    const double *v_work;        // [batch][n]      v after the (optional) projection
    const int *tight_cnt;        // [batch][n]      tight edges per row
    const uint32_t *tight_bits;  // [batch][n][W]   tight-edge bitmap per row, W = ceil(n/32)
    const int *inst_flags;       // [batch]
    double tight_eps;
    // outputs
    long long *x_out, *y_out;  // [batch][n] int64 (seeded API) or null
    int *x32_out, *y32_out;    // [batch][n] int32 (lapjv API) or null
    double *v_out;             // [batch][n] final column duals or null
    double *u_out;             // [batch][n] u_i = C[i][x_i] - v[x_i] or null
    int *ret;                  // [batch]
    long long *stats;          // [batch][kStatsPerInstance] (StatSlot) or null
    // per-instance state in global memory, only used when the state does not fit LDS
    double *g_dist, *g_v;
    int *g_order, *g_pred, *g_y, *g_x, *g_fr, *g_evl, *g_tmpcol;
    // helper workgroups (phase-0 launches of seeded solves; LAPWARM_HELPER=0 turns them off):
    // [batch][kRingInts] ring of upcoming head rows, zeroed by the caller; word 0 = done flag,
    // words 2.. = (generation << 16 | row)
    int *pf_ring;
    int helper;  // helper workgroups per instance (0: none)
    // cooperative shortest-path phase (coop_ssp.hip): phase 0 = the whole solve in this kernel;
    // 1 = stop before the shortest-path phase and leave x, y, v, the free-row list in the global
    // state arrays + the hand-over block; 2 = take x, y, v back, run the paths the cooperative kernel
    // left (hand[kHandPathsDone] .. hand[kHandFreeRows]) and write the outputs; 3 = between two launches of the
    // cooperative kernel: run the one path it stopped at
    int phase;
    int *hand;                 // [batch][kHandInts] (HandSlot)
    long long *cstats;         // [batch][kCoopStats] (CoopStat)
    unsigned long long *mail;  // [batch][mail_granules] zeroed by phase 1
    int mail_granules;
    // candidate lists of the augmenting row reduction (cold solves, lapwarm_lapjv_*_batched):
    // [batch][n][kArrListEntries] raw costs / columns, [batch][n] thresholds; null = plain row scans
    // (last: a member in the middle moved the kernel arguments behind it and cost the seeded kernel 12 SGPR spills)
    double *arr_lval, *arr_ltau;
    int *arr_lcol;
};
constexpr int kArrListEntries = 128;
constexpr int kRingSlots = 64;
constexpr int kRingInts = 2 + kRingSlots;

struct CoopParams {
    const double *C;
    int n, batch;
    int G;             // members (single-wave workgroups) per instance, filled in by launch_coop
    int first, count;  // instances [first, first + count) of this launch
    int xcd_stores;    // allow workgroup-scope mailbox stores when all members of an instance share an XCD
    double *v;         // [batch][n] column duals (the solver's global state arrays)
    int *x, *y, *pred;
    const int *fr;     // [batch][n] free rows, hand[kHandFreeRows] of them
    int *hand;
    long long *cstats;
    unsigned long long *mail;
};

// ---- the solve plan (jv_solver.hip: plan_solve): every host decision about how a solve runs ---------
// The workspace layout (lapwarm_abi.hip) and the ABI queries ask the same functions.
enum class SolveShape {
    kOneLaunch,       // phase 0: the whole solve in one launch of jv_instance_kernel
    kListsThenPaths,  // phase 1 with candidate lists (cold), then phase 2
    kCoopChain,       // phase 1, (coop_ssp_kernel, phase 3) x pairs, coop_ssp_kernel, phase 2
};
SolveShape solve_shape(int n, bool lists);  // lists: the workspace carries candidate lists (cold solves)

struct PhaseConfig {  // one launch of jv_instance_kernel<ch, ldsl, tb, lists>
    int threads, ch, ldsl, tb;
    bool lists;
    size_t lds_bytes;
};

// coop_ssp_kernel<ch, nl> (coop_ssp.hip); members == 0: no cooperative path for this size
struct CoopConfig {
    int ch, nl, members;   // members: single-wave workgroups per instance
    size_t mail_granules;  // per instance
    int per_launch;        // instances per launch
    int pairs;             // (cooperative, phase 3) pairs before the final cooperative launch
    int xcd_stores;
};
CoopConfig coop_config(int n);
hipError_t launch_coop(const CoopParams &p, const CoopConfig &cfg, hipStream_t stream);

struct SolvePlan {
    SolveShape shape;
    PhaseConfig prep;   // phase 0, or phase 1
    PhaseConfig paths;  // phases 2 and 3
    int helper;         // helper workgroups per instance (phase 0 only)
    CoopConfig coop;
};
SolvePlan plan_solve(int mode, int batch, int n, int threads_hint, bool lists, int n_cus);
hipError_t launch_solver(const SolvePlan &plan, const SolverParams &p, hipStream_t stream);

size_t solver_lds_bytes(int n, int ch, int level);
int solver_lds_level(int n, int ch);
bool solver_needs_global_state(int n);
// candidate lists for the augmenting row reduction: from the size where a row is a few times its list
// (LAPWARM_ARR_LISTS=0 turns them off: every iteration then scans its whole row)
bool arr_lists_enabled(int n);
bool solver_uses_helpers(int n);  // seeded mode: one helper workgroup per instance of a phase-0 launch

// ---- dense sweeps (dense_sweeps.hip) ----------------------------------------------------
struct PreludeParams {
    const double *C;
    int n, batch;
    const double *u;  // [batch][n] duals the verify step uses (seed, or projected)
    const double *v;  // [batch][n]
    double eps, tight_eps;
    int rerun;        // 0: first pass; 1: only instances whose duals were projected
    double *u_tight;
    int *viol_cnt;    // [batch][n] candidates of the projection per row (first pass only)
    int *tight_cnt;
    uint32_t *tight_bits;
    int *inst_flags;
};
hipError_t launch_prelude(const PreludeParams &p, hipStream_t stream);
hipError_t launch_seed_prepare(const double *u_seed, const double *v_seed, double *u_work, double *v_work,
                               size_t count, int *flags, int n_flags, int *ring, int n_ring, hipStream_t stream);

// Gauss-Seidel projection of (u, v) for the instances flagged kFlagHasViolation; in place.
hipError_t launch_projection(const double *C, int n, int batch, double *u, double *v,
                             const int *viol_cnt, int *inst_flags, double eps, hipStream_t stream);

// out[b][j] = min_i (C[b][i][j] - (u ? u[b][i] : 0)); `partial` holds batch*chunks*n doubles.
int colmin_chunks(int n, int batch);
hipError_t launch_colmin(const double *C, int n, int batch, const double *u, double *out,
                         double *partial, hipStream_t stream);

// out[b][i] = min_j (C[b][i][j] - (v ? v[b][j] : 0))
hipError_t launch_rowmin(const double *C, int n, int batch, const double *v, double *out,
                         hipStream_t stream);

// R[b][i][j] = (C - u_i) - v_j - shift[b] ; gmin[b] = min_ij ((C - u_i) - v_j)
hipError_t launch_reduced_min(const double *C, int n, int batch, const double *u, const double *v,
                              double *gmin_partial, double *gmin, hipStream_t stream);
hipError_t launch_reduce_costs(const double *C, int n, int batch, const double *u, const double *v,
                               const double *gmin, int shift_nonneg, double *out, hipStream_t stream);
// one round of project_feasible's u/v caps: u = min(u, rowmin(C - v)) ; v = min(v, colmin(C - u))
hipError_t launch_cap_rows(const double *C, int n, int batch, double *u, const double *v,
                           hipStream_t stream);
hipError_t launch_cap_cols(const double *C, int n, int batch, const double *u, double *v,
                           double *partial, hipStream_t stream);

// 13 row statistics + 8 positional encodings (float32) and the 16 smallest costs per row.
struct FeatureParams {
    const double *C;
    int n, batch;
    const double *colmin;  // [batch][n]
    const float *posenc;   // [n][8] host-computed table
    float *feat;           // [batch][n][21]
    float *topk;           // [batch][n][16] ascending, +inf padded, or null
};
hipError_t launch_row_features(const FeatureParams &p, hipStream_t stream);

// ---- oracle duals (oracle_duals.hip) ----------------------------------------------------
constexpr int kOracleMaxN = 16384;
constexpr int kOracleReplayMaxN = 2048;  // largest n whose unsettled instances are replayed exactly
// per-instance results (the ret codes of lapwarm_oracle_duals_batched) and internal states
constexpr int kOracleOk = 0, kOracleNegativeCycle = 1, kOracleInfeasible = 2, kOracleSlackness = 3,
              kOracleNotPermutation = 4, kOracleNonFinite = 5;
constexpr int kOracleDone = 100, kOracleReplay = 101;  // status 0: still sweeping
// per-instance int slots of the workspace
constexpr int kOdStatus = 0, kOdCount0 = 1, kOdCount1 = 2, kOdSweeps = 3, kOdDepth = 4, kOdRowsRead = 5,
              kOdReplayed = 6, kOdSlackBad = 7, kOdInstInts = 16;
struct OracleParams {
    const double *C;
    int n, batch, chunks, pair;
    const int *rows, *cols;  // [batch][n] pairs in the caller's order
    int *x, *y;              // [batch][n] row -> col, col -> row
    double *cxx;             // [batch][n] C[i][x_i]
    double *v0, *v1;         // [batch][n] the two Jacobi buffers
    int *pred;               // [batch][n] row that last lowered v_j, or -1
    int *lrow;               // [2][batch][n] active rows of the current / next sweep
    double *lsrc;            // [2][batch][n] their source values v[x_i]
    double *pval;            // [batch][chunks][n] partial column minima
    int *parg;               // [batch][chunks][n] their rows
    int *inst;               // [batch][kOdInstInts]
};
int oracle_chunks(int n, int batch);
hipError_t launch_oracle_init(const OracleParams &p, hipStream_t stream);
// sweep s (0-based, the same for every instance of the batch)
hipError_t launch_oracle_sweep(const OracleParams &p, int s, hipStream_t stream);
// after s sweeps: stop the converged, find predecessor cycles; `last` hands the unsettled to the
// replay; `running` (zeroed by the caller) receives the number of instances that go on sweeping
hipError_t launch_oracle_check(const OracleParams &p, int s, int last, int *running, hipStream_t stream);
// replay (n <= kOracleReplayMaxN), u/v with the gauge, reduced-cost minimum, ret and counters
hipError_t launch_oracle_finish(const OracleParams &p, double tol, double *u, double *v, double *rowpart,
                                double *gmin, int *ret, int *sweeps, hipStream_t stream);

// ---- rectangular / cost-limited lapjv (extend_costs.hip) -----------------------------------
// E [batch][n][n] = C [batch][n_rows][n_cols] in the top left corner, `fill` beside and below it,
// 0 in E[n_rows:, n_cols:] (LAP/_lapjv_cpp/_lapjv.pyx:84-95; fill = 0 without a cost limit)
hipError_t launch_extend_costs(const double *C, int batch, int n_rows, int n_cols, int n, double fill, double *E,
                               hipStream_t stream);
// _lapjv.pyx:115-122: xs, ys [batch][n] of the solve on E -> x [batch][n_rows], y [batch][n_cols] with -1
// for unmatched, matched [batch] and opt [batch] (either may be null); gath [batch][n_rows] scratch.
// Instances with ret != 0: x, y all -1, opt NaN, matched 0.
hipError_t launch_extended_finish(const double *C, int batch, int n_rows, int n_cols, int n, const int *xs,
                                  const int *ys, const int *ret, int *x, int *y, double *opt, int *matched,
                                  double *gath, hipStream_t stream);

// OneGNN refinement aggregation (onegnn_refine.hip)
hipError_t launch_refine_aggregate(const float *topk16, const float *u_pre, const float *w1,
                                   const float *b1, float *out, float *wsum, int rows, int H,
                                   hipStream_t stream);

}  // namespace lapwarm
