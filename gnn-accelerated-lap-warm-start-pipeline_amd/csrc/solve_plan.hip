// solve_plan.hip -- the host side of a solve: the environment knobs, the planning rules (geometry, LDS
// level, helpers, candidate lists, cooperative chain) and the launch sequence that runs a plan.  No kernel
// and nothing bound to a template instantiation: the launch tables stay with their kernels
// (jv_solver.hip: launch_phase, coop_ssp.hip: launch_coop), so an edit here recompiles neither.
#include <stdlib.h>

#include "solve_plan.hpp"

namespace lapwarm {

namespace {

// The LAPWARM_* environment switches, read once per process (knobs()).  All default to the
// measured-best setting.
struct Knobs {
    int arr_lists;             // LAPWARM_ARR_LISTS=0: cold solves scan whole rows instead of candidate lists
    int helper;                // LAPWARM_HELPER=0: no helper workgroups beside seeded phase-0 launches
    int helper_max_n;          // LAPWARM_HELPER_MAX_N: largest n that gets helper workgroups
    int helpers_per_instance;  // LAPWARM_HELPERS_PER_INSTANCE: helper workgroups per instance, 1..4 (tested: 2, 4)
    int coop;                  // LAPWARM_COOP=0: never plan the cooperative shortest-path kernel
    int coop_min_n;            // LAPWARM_COOP_MIN_N: smallest n that takes the cooperative chain (tested: 1)
    int coop_ch;               // LAPWARM_COOP_CH: forced positions per lane {1,2,4,8,16} (0: by size) (tested: all)
    int coop_xcd_stores;       // LAPWARM_COOP_XCD_STORES=0: mailbox stores stay agent-scope on one XCD (tested)
    int coop_relaunches;       // LAPWARM_COOP_RELAUNCHES: (cooperative, phase 3) pairs per solve, 0..4096 (tested: 0, 1)
    // "tested": tests/test_gpu_coop_instantiations.py sweeps the setting against the oracle
};

int env_switch(const char *name)  // on unless the first character is '0'
{
    const char *e = getenv(name);
    return (e && e[0] == '0') ? 0 : 1;
}

int env_int(const char *name, int unset)
{
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
}

const Knobs &knobs()
{
    static const Knobs k = [] {
        Knobs k;
        k.arr_lists = env_switch("LAPWARM_ARR_LISTS");
        k.helper = env_switch("LAPWARM_HELPER");
        k.helper_max_n = env_int("LAPWARM_HELPER_MAX_N", 8192);  // n = 16384: 29.3 s with a helper against 25.6 s without
        const int h = env_int("LAPWARM_HELPERS_PER_INSTANCE", 1);
        k.helpers_per_instance = (h >= 1 && h <= 4) ? h : 1;
        k.coop = env_switch("LAPWARM_COOP");
        // default: sizes whose solver state no longer fits one CU's LDS (solver_lds_level 0); below that the
        // single-workgroup kernel is faster (n = 4096: 274 ms against 442 ms per 32 instances)
        k.coop_min_n = env_int("LAPWARM_COOP_MIN_N", 4428);
        k.coop_ch = env_int("LAPWARM_COOP_CH", 0);
        k.coop_xcd_stores = env_switch("LAPWARM_COOP_XCD_STORES");
        const int r = env_int("LAPWARM_COOP_RELAUNCHES", 96);
        k.coop_relaunches = (r >= 0 && r <= 4096) ? r : 96;
        return k;
    }();
    return k;
}

// Positions per lane for a problem size: enough members to spread the row over many CUs, few
// enough that one exchange stays within four granule loads per lane (G <= 32).
int coop_ch(int n)
{
    const int forced = knobs().coop_ch;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16) {
        if ((n + 64 * forced - 1) / (64 * forced) <= 32) return forced;
    }
    // Measured (tools/micro/hop_bench.hip, profiles/r03_hop_bench.txt): an exchange among 8 members costs
    // 1.0-1.3 us, among 16 1.4-2.2 us (32 instances in flight), among 32 1.9-2.6 us -- the fewer members the
    // better, as long as a lane's positions fit the register file (16 positions = ~250 VGPRs).
    if (n <= 512) return 1;
    if (n <= 1024) return 2;
    // Measured with one event per member in a 2-granule relax record (a relax round polls 2G + 24 granules:
    // one load per lane up to 20 members, two up to 32): n = 4608 x 8 467 ms with 4 positions per lane
    // (18 members) against 508 ms with 8; n = 8192 1.13 s with 4 (32 members), 1.21 s with 8, 1.59 s with 16;
    // n = 16384 3.88 s with 8 (32 members), 4.75 s with 16.
    if (n <= 8192) return 4;
    return 8;
}

}  // namespace

CoopConfig coop_config(int n)
{
    const Knobs &kn = knobs();
    CoopConfig c = {};
    if (!kn.coop || n < kn.coop_min_n || n > 16384) return c;
    const int ch = coop_ch(n);
    const int members = (n + 64 * ch - 1) / (64 * ch);
    const int nl = coop_granule_loads(members);
    // (a forced geometry without an instantiation takes the one-workgroup path)
    if (members > 32 || !coop_kernel_exists(ch, nl)) return c;
    c.ch = ch;
    c.nl = nl;
    c.members = members;
    c.mail_granules = coop_mail_granules(members);
    // every member of an instance must be resident while the instance runs: at most 1024 single-wave
    // workgroups per launch (a quarter of what the chip holds), instances in groups of 8
    c.per_launch = (1024 / members) & ~7;
    if (c.per_launch < 8) c.per_launch = 8;
    c.pairs = kn.coop_relaunches;
    c.xcd_stores = kn.coop_xcd_stores;
    return c;
}

bool arr_lists_enabled(int n) { return knobs().arr_lists && n >= 512; }

// n = 8192 -> 512 threads x 16 positions, two row slots.  Measured (uniform instance, ms per solve):
// n = 8192: 2,278 here against 2,658 with 1024 x 8 and the state in global memory (level 0);
// n = 16384 (512 x 32, one slot): 51 s against 25 s for 1024 x 16 at level 0 -- the step time grows
// with the positions per thread, so K5 stays on the generic path.
bool large_row_geometry(int n, int *threads, int *ch)
{
    if (n != 8192) return false;
    *threads = 512;
    *ch = n / 512;
    return solver_row_slots(n, *ch) >= 1;
}

// LDS levels: 2 = position-owned search, every array in LDS; 1 = x and the free-row list in global
// memory; 0 = all global; 8 = all global + head rows staged in LDS row slots (solver_lds_bytes).
int solver_lds_level(int n, int ch)
{
    if (solver_lds_bytes(n, ch, 2) <= kLdsBudgetBytes) return 2;
    if (solver_lds_bytes(n, ch, 1) <= kLdsBudgetBytes) return 1;
    return 0;
}

// Picks (threads, CH) with threads*CH >= n.  `threads_hint` (0 = auto) lets the bench sweep
// the geometry; it is rounded to a supported value.
static void solver_geometry(int n, int threads_hint, int *threads, int *ch)
{
    int t = threads_hint;
    if (t <= 0) {
        // measured on MI355X (K3, n=2048): 1024 threads 107 ms, 512: 128 ms, 256: 180 ms --
        // the per-step fixed latency dominates, so use as many lanes as there are columns
        if (n <= 64) t = 64;
        else if (n <= 128) t = 128;
        else if (n <= 256) t = 256;
        else if (n <= 512) t = 512;
        else t = 1024;
    }
    t = ((t + 63) / 64) * 64;
    if (t > 1024) t = 1024;
    if (t < 64) t = 64;
    int c = 1;
    while ((long long)t * c < n && c < 16) c <<= 1;
    while ((long long)t * c < n && t < 1024) t += 64;
    *threads = t;
    *ch = c;
}

// Helper workgroups: rows of 8-64 KiB (n = 1024 .. 8192, even).  Measured on the same box, solver
// kernel per launch: K3 79.6 -> 73.2 ms, K4 slice 327.8 -> 276.0 ms, n = 8192 2.28 -> 2.09 s,
// K2 (n = 512) no change, n = 16384 worse.
bool solver_uses_helpers(int n)
{
    const Knobs &kn = knobs();
    return kn.helper && n >= 1024 && n <= kn.helper_max_n && n % 2 == 0;
}

SolveShape solve_shape(int n, bool lists)
{
    if (coop_config(n).members > 0) return SolveShape::kCoopChain;
    return lists ? SolveShape::kListsThenPaths : SolveShape::kOneLaunch;
}

SolvePlan plan_solve(int mode, int batch, int n, int threads_hint, bool lists, int n_cus)
{
    SolvePlan plan = {};
    plan.shape = solve_shape(n, lists);
    if (plan.shape == SolveShape::kCoopChain) plan.coop = coop_config(n);
    PhaseConfig &k = plan.paths;
    // measured (n=2048, ARR-dominated cold solve): 512 threads 2.6 us/iteration, 1024: 3.2, 256: 3.1
    if (threads_hint <= 0 && mode == kModeCold && n > 1024 && n <= 2048) threads_hint = 512;
    solver_geometry(n, threads_hint, &k.threads, &k.ch);
    // Rows that no longer fit the L1 (n > 4,427, where the state leaves LDS as well): 512 threads
    // with n/512 positions each -- duals cached in registers (256 VGPRs per thread at this size),
    // every head row brought into LDS by coalesced LDS-DMA (level 8).  Seeded mode only: the cold
    // ARR loop keeps the generic geometry.
    if (threads_hint <= 0 && mode == kModeSeeded && large_row_geometry(n, &k.threads, &k.ch)) {
        k.ldsl = 8;
        k.tb = 512;
    } else {
        k.ldsl = solver_lds_level(n, k.ch);
        k.tb = k.threads <= 256 ? 256 : 1024;
    }
    k.lds_bytes = solver_lds_bytes(n, k.ch, k.ldsl);
    // a cold solve whose workspace carries the candidate lists is prepared by the LISTS instantiation
    plan.prep = k;
    plan.prep.lists = lists;
    const int n_helpers = knobs().helpers_per_instance;
    // (a helper can only help while its solver runs: with more workgroups than CUs the helpers would
    // be dispatched after the solvers they serve and leave at once -- skip them.  Assumptions, stated:
    // workgroups are dispatched in index order, so every solver of THIS launch is resident before its
    // helper; a helper spins until its solver's done flag or 0.5 s (60 s above n = 4096) and holds a
    // CU's LDS meanwhile, so with several launches resident -- bench.py --inflight -- helpers can delay
    // the solvers of a later launch, never deadlock them: every solver exit sets the flag.)
    if (plan.shape == SolveShape::kOneLaunch && mode == kModeSeeded && solver_uses_helpers(n) &&
        batch * (1 + n_helpers) <= n_cus)
        plan.helper = n_helpers;
    return plan;
}

// Runs a plan: one launch of jv_instance_kernel, or phase 1 (greedy / micro-ARR / cold preparation),
// the cooperative chain where the plan has one, then phase 2 (whatever is left + the outputs).
hipError_t launch_solver(const SolvePlan &plan, const SolverParams &p_in, hipStream_t stream)
{
    SolverParams p = p_in;
    p.helper = plan.helper;
    p.mail_granules = (int)plan.coop.mail_granules;
    if (plan.shape == SolveShape::kOneLaunch) {
        p.phase = 0;
        return launch_phase(plan.prep, p, stream);
    }
    p.phase = 1;
    hipError_t e = launch_phase(plan.prep, p, stream);
    if (e != hipSuccess) return e;
    if (plan.shape == SolveShape::kCoopChain) {
        CoopParams c = {};
        c.C = p.C;
        c.n = p.n;
        c.batch = p.batch;
        c.v = p.g_v;
        c.x = p.g_x;
        c.y = p.g_y;
        c.pred = p.g_pred;
        c.fr = p.g_fr;
        c.hand = p.hand;
        c.cstats = p.cstats;
        c.mail = p.mail;
        // The cooperative kernel stops at a path it does not handle (a minima collection with a tie: rare,
        // but seeds that went through float32 produce a few dozen per instance); jv_instance_kernel then
        // searches that ONE path (phase 3) and the cooperative kernel carries on.  The host cannot know how
        // often that happens, so a fixed number of (cooperative, one-path) pairs is enqueued -- a launch with
        // nothing to do returns at once (~2 us) -- and the final phase 2 finishes whatever is left.
        for (int k = 0; k <= plan.coop.pairs; ++k) {
            e = launch_coop(c, plan.coop, stream);
            if (e != hipSuccess) return e;
            if (k == plan.coop.pairs) break;
            p.phase = 3;
            e = launch_phase(plan.paths, p, stream);
            if (e != hipSuccess) return e;
        }
    }
    p.phase = 2;
    return launch_phase(plan.paths, p, stream);
}

bool ragged_solve_eligible(int n)
{
    if (n < 1 || n > 16384) return false;
    return solve_shape(n, false) == SolveShape::kOneLaunch && !solver_uses_helpers(n) && !solver_needs_global_state(n);
}

// A cold instance of a ragged launch: one launch, all state in LDS, no candidate lists (the RAGGED
// instantiations are compiled without them), and a (CH, TB) that launch_phase_ragged has.
bool ragged_cold_eligible(int n)
{
    if (n < 1 || n > 16384 || arr_lists_enabled(n)) return false;
    const SolvePlan plan = plan_solve(kModeCold, 1, n, 0, false, 0);
    const PhaseConfig &k = plan.prep;
    if (plan.shape != SolveShape::kOneLaunch || k.ldsl != 2 || plan.helper != 0) return false;
    return k.tb == 1024 ? (k.ch == 1 || k.ch == 2 || k.ch == 4) : (k.tb == 256 && k.ch == 1);
}

static int plan_groups(int mode, const int *sizes, int batch, int *group_of, RaggedGroup *groups)
{
    int count = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = sizes[b];
        if (!(mode == kModeCold ? ragged_cold_eligible(n) : ragged_solve_eligible(n))) return -1;
        // (batch and the CU count only decide about helpers, which an eligible size does not have)
        const PhaseConfig k = plan_solve(mode, batch, n, 0, false, 0).prep;
        int g = 0;
        for (; g < count; ++g) {
            const PhaseConfig &q = groups[g].k;
            if (q.threads == k.threads && q.ch == k.ch && q.ldsl == k.ldsl && q.tb == k.tb && q.lists == k.lists) break;
        }
        if (g == count) {
            if (count == kMaxRaggedGroups) return -1;
            groups[count++] = RaggedGroup{k, n, n};
        } else {
            RaggedGroup &r = groups[g];
            if (k.lds_bytes > r.k.lds_bytes) r.k.lds_bytes = k.lds_bytes;
            if (n < r.n_lo) r.n_lo = n;
            if (n > r.n_hi) r.n_hi = n;
        }
        if (group_of) group_of[b] = g;
    }
    for (int g = 0; g < count; ++g) {
        for (int h = g + 1; h < count; ++h) {
            if (groups[g].n_lo <= groups[h].n_hi && groups[h].n_lo <= groups[g].n_hi) return -1;
        }
    }
    return count;
}

int plan_ragged_groups(const int *sizes, int batch, int *group_of, RaggedGroup *groups)
{
    return plan_groups(kModeSeeded, sizes, batch, group_of, groups);
}

int plan_ragged_groups_cold(const int *sizes, int batch, int *group_of, RaggedGroup *groups)
{
    return plan_groups(kModeCold, sizes, batch, group_of, groups);
}

bool solver_needs_global_state(int n)
{
    // a threads_hint may pick another CH: be conservative for every supported geometry.
    // Level 2 keeps everything in LDS; 0, 1 and 8 use the global workspace.
    for (int c = 1; c <= 16; c <<= 1) {
        if (solver_lds_level(n, c) < 2) return true;
    }
    int t, c;
    if (large_row_geometry(n, &t, &c)) return true;
    return false;
}

}  // namespace lapwarm
