// solve_plan.hpp -- the solve plan (solve_plan.hip): every host decision about how a solve runs.
// The workspace layout (lapwarm_abi.hip) and the ABI queries ask the same functions.  Host only: the
// kernels and their launch tables are behind jv_solver.hpp.
#pragma once

#include "jv_solver.hpp"

namespace lapwarm {

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

struct SolvePlan {
    SolveShape shape;
    PhaseConfig prep;   // phase 0, or phase 1
    PhaseConfig paths;  // phases 2 and 3
    int helper;         // helper workgroups per instance (phase 0 only)
    CoopConfig coop;
};
SolvePlan plan_solve(int mode, int batch, int n, int threads_hint, bool lists, int n_cus);
hipError_t launch_solver(const SolvePlan &plan, const SolverParams &p, hipStream_t stream);

// ---- seeded solves of a ragged batch (lapwarm_seeded_ragged): one launch per kernel configuration ----
// An instance is eligible when its own plan is one launch without helper workgroups and with all state in
// LDS: solve_shape kOneLaunch, solver_uses_helpers and solver_needs_global_state both false.
bool ragged_solve_eligible(int n);
// Instances share a launch when their plans have the same PhaseConfig template arguments and workgroup size
// (threads, ch, ldsl, tb, lists); the launch's dynamic LDS is the largest of the group.  Every rule of the plan
// is monotone in n, so a group is the eligible sizes of an interval [n_lo, n_hi]: that is how a workgroup
// tells, from sizes[b] alone, whether a launch is its own (plan_ragged_groups checks that the intervals of
// one call are disjoint).
struct RaggedGroup {
    PhaseConfig k;
    int n_lo, n_hi;  // smallest and largest size of the call in this group
};
constexpr int kMaxRaggedGroups = 16;
// Groups in the order of their first instance; group_of [batch] (may be null) receives each instance's group.
// Returns the number of groups, -1 when an instance is not eligible (or there are more than
// kMaxRaggedGroups configurations, or two intervals overlap: neither happens with the rules above).
int plan_ragged_groups(const int *sizes, int batch, int *group_of, RaggedGroup *groups);

// ---- cold solves of a ragged batch (lapwarm_lapjv_ragged, lapwarm_lapjv_extended_ragged) ----
// Eligible: the instance's own cold plan (plan_solve(kModeCold, ..), no threads hint) is one launch at LDS
// level 2 without helper workgroups, and arr_lists_enabled(n) is false: every n <= 511 with the default
// settings; LAPWARM_ARR_LISTS=0 widens the class to where the state leaves LDS.  Groups as above, by the
// PhaseConfig of the cold plan (so 1024 < n <= 2048 gets the 512-thread geometry it gets alone).
bool ragged_cold_eligible(int n);
int plan_ragged_groups_cold(const int *sizes, int batch, int *group_of, RaggedGroup *groups);

int solver_lds_level(int n, int ch);
bool solver_needs_global_state(int n);
// candidate lists for the augmenting row reduction: from the size where a row is a few times its list
// (LAPWARM_ARR_LISTS=0 turns them off: every iteration then scans its whole row)
bool arr_lists_enabled(int n);
bool solver_uses_helpers(int n);  // seeded mode: one helper workgroup per instance of a phase-0 launch

}  // namespace lapwarm
