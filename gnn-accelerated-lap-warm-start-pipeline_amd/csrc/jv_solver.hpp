// jv_solver.hpp -- host-visible interface of the solver kernels: the per-instance kernel (jv_solver.hip)
// and the cooperative shortest-path kernel (coop_ssp.hip).  Internal to the shared library; the
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
    // a launch of the ragged seeded solve (launch_phase_ragged; appended for the same reason): a grid of `batch`
    // workgroups, workgroup b runs instance b when rg_n_lo <= rg_sizes[b] <= rg_n_hi.  n is not read then.
    const long long *rg_offsets;  // [batch] element offset of the matrix in C, device
    const int *rg_sizes;          // [batch] n_b, device
    int rg_ld;                    // row stride, 0: n_b
    int rg_N;                     // stride of the [batch][.] seeded inputs and outputs
    int rg_n_lo, rg_n_hi;
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

// ---- launchers (the plan they run is solve_plan.hpp's; the launch tables are private to the kernel files) ----
struct PhaseConfig;
struct CoopConfig;
hipError_t launch_phase(const PhaseConfig &k, const SolverParams &p, hipStream_t stream);  // jv_instance_kernel
hipError_t launch_phase_ragged(const PhaseConfig &k, const SolverParams &p, hipStream_t stream);  // its RAGGED form
hipError_t launch_coop(const CoopParams &p, const CoopConfig &cfg, hipStream_t stream);    // coop_ssp_kernel

// the LDS carving of jv_instance_kernel (jv_solver.hip): bytes of a level, row slots of level 8
size_t solver_lds_bytes(int n, int ch, int level);
__host__ __device__ int solver_row_slots(int n, int ch);

// what the plan needs from coop_ssp.hip's private record sizes, per member count of an instance
bool coop_kernel_exists(int ch, int nl);  // is there a coop_ssp_kernel<ch, nl>
int coop_granule_loads(int members);      // granule loads per lane (nl)
size_t coop_mail_granules(int members);   // mailbox granules per instance

}  // namespace lapwarm
