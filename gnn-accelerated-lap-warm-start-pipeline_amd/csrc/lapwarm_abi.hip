// lapwarm_abi.hip -- the C ABI of liblapwarm_hip.so (declared in include/lapwarm_hip.h).
//
// Host-pointer entry points stage through a grow-only device arena and call the batched
// device entry points with batch = 1; the batched entry points only enqueue work on the
// caller's stream (no allocation, no synchronisation).
#include <hip/hip_runtime.h>

#include <math.h>
#include <mutex>
#include <stdio.h>
#include <string.h>
#include <tuple>
#include <vector>

#include "../../include/lapwarm_hip.h"
#include "cost_families.hpp"
#include "dense_sweeps.hpp"
#include "dual_gnn.hpp"
#include "extend_costs.hpp"
#include "extend_ragged.hpp"
#include "graph_features.hpp"
#include "jv_solver.hpp"
#include "lapmod_sparse.hpp"
#include "onegnn_refine.hpp"
#include "oracle_duals.hpp"
#include "prune_price.hpp"
#include "ragged_batch.hpp"
#include "ragged_duals.hpp"
#include "solve_plan.hpp"
#include "train_loss.hpp"

using namespace lapwarm;

namespace {

thread_local char g_err[256] = "";

int fail(hipError_t e, const char *where)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return -1000 - (int)e;
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return fail(_e, #expr);   \
    } while (0)

// The one workspace check of every entry point that takes one.
int check_workspace(size_t have, size_t need)
{
    if (have >= need) return 0;
    snprintf(g_err, sizeof(g_err), "workspace too small: %zu < %zu", have, need);
    return -1;
}

hipStream_t as_stream(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carver {
    unsigned char *base;
    size_t off;
    template <typename T>
    T *take(size_t count)
    {
        T *p = reinterpret_cast<T *>(base + off);
        off += align_up(sizeof(T) * count);
        return p;
    }
};

// ---- workspace layouts: one function per kind; a null base measures the workspace ----------

// The seeded prelude's buffers, [batch][stride] each but the flags [batch].  The tight-edge bitmap of instance b
// is n_b rows of ceil(n_b / 32) words at b * stride * ceil(stride / 32).
struct PreludeWs {
    double *u_work, *v_work, *u_tight;
    int *viol_cnt, *tight_cnt, *flags;
    uint32_t *tight_bits;
};

PreludeWs prelude_layout(Carver &c, int batch, int stride)
{
    PreludeWs w;
    const size_t bn = (size_t)batch * stride;
    w.u_work = c.take<double>(bn);
    w.v_work = c.take<double>(bn);
    w.u_tight = c.take<double>(bn);
    w.viol_cnt = c.take<int>(bn);
    w.tight_cnt = c.take<int>(bn);
    w.flags = c.take<int>((size_t)batch);
    w.tight_bits = c.take<uint32_t>(bn * ((size_t)(stride + 31) / 32));
    return w;
}

// The solver workspace of a seeded or a cold solve, laid out into the kernel argument block (the
// caller adds C and its results).  Its size depends on neither the mode nor the threads hint: the
// global solver state is carved whenever any geometry of this size needs it.
struct SolverWs {
    SolverParams sp;
    PreludeWs pre;
    bool lists;  // carries the candidate lists of the cold row reduction
    size_t bytes;
};

// what the prelude leaves for the solver (seeded_prelude adds tight_eps)
void hand_prelude_to_solver(const PreludeWs &pre, SolverParams *sp)
{
    sp->u_tight = pre.u_tight;
    sp->v_work = pre.v_work;
    sp->tight_cnt = pre.tight_cnt;
    sp->tight_bits = pre.tight_bits;
    sp->inst_flags = pre.flags;
}

SolverWs solver_layout(void *ws, int batch, int n, int mode, bool with_lists)
{
    SolverWs w;
    SolverParams &sp = w.sp;
    memset(&sp, 0, sizeof(sp));
    sp.n = n;
    sp.batch = batch;
    sp.mode = mode;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    const size_t bn = (size_t)batch * n;
    w.lists = with_lists && arr_lists_enabled(n);
    const SolveShape shape = solve_shape(n, w.lists);
    w.pre = prelude_layout(c, batch, n);
    sp.pf_ring = c.take<int>((size_t)batch * kRingInts);
    // a two-phase solve hands the state from phase 1 to the later launches through these
    if (shape != SolveShape::kOneLaunch) {
        sp.hand = c.take<int>((size_t)batch * kHandInts);
        sp.cstats = c.take<long long>((size_t)batch * kCoopStats);
    }
    if (shape == SolveShape::kCoopChain)
        sp.mail = c.take<unsigned long long>((size_t)batch * coop_config(n).mail_granules);
    if (solver_needs_global_state(n) || shape != SolveShape::kOneLaunch) {
        sp.g_dist = c.take<double>(bn);
        sp.g_v = c.take<double>(bn);
        sp.g_order = c.take<int>(bn);
        sp.g_pred = c.take<int>(bn);
        sp.g_y = c.take<int>(bn);
        sp.g_x = c.take<int>(bn);
        sp.g_fr = c.take<int>(bn);
        sp.g_evl = c.take<int>(bn);
        sp.g_tmpcol = c.take<int>(bn + 2 * (size_t)batch);
    }
    // candidate lists of the augmenting row reduction (jv_solver.hip, cold_arr_sweep): 1,544 bytes per row
    if (w.lists) {
        sp.arr_lval = c.take<double>(bn * kArrListEntries);
        sp.arr_lcol = c.take<int>(bn * kArrListEntries);
        sp.arr_ltau = c.take<double>(bn);
    }
    w.bytes = c.off;
    if (mode == kModeSeeded)
        hand_prelude_to_solver(w.pre, &sp);
    else
        sp.pf_ring = nullptr;  // a cold solve starts from C alone
    return w;
}

// The seeded solve of a ragged batch: the prelude's buffers with the padded stride N.  Nothing else: an
// instance this entry takes keeps its solver state in LDS and has no helper ring.
struct RaggedSolverWs {
    PreludeWs pre;
    size_t bytes;
};

RaggedSolverWs ragged_solver_layout(void *ws, int batch, int N)
{
    RaggedSolverWs w;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    w.pre = prelude_layout(c, batch, N);
    w.bytes = c.off;
    return w;
}

// The dense sweeps: column-min partials, column minima, row partials.
struct SweepWs {
    double *partial, *colmin, *rowpart;
    size_t bytes;
};

SweepWs sweep_layout(void *ws, int batch, int n)
{
    SweepWs s;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    const size_t bn = (size_t)batch * n;
    s.partial = c.take<double>(bn * (size_t)colmin_chunks(n, batch));
    s.colmin = c.take<double>(bn);
    s.rowpart = c.take<double>(bn);
    s.bytes = c.off;
    return s;
}

// Oracle duals: the buffers of OracleParams, then the finish step's and the sweep loop's.
struct OracleWs {
    double *rowpart, *gmin;
    int *running;
    size_t bytes;
};

OracleWs oracle_layout(void *ws, int batch, int n, OracleParams *p)
{
    OracleWs s;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    const size_t bn = (size_t)batch * n;
    const size_t chunks = (size_t)oracle_chunks(n, batch);
    p->x = c.take<int>(bn);
    p->y = c.take<int>(bn);
    p->pred = c.take<int>(bn);
    p->cxx = c.take<double>(bn);
    p->v0 = c.take<double>(bn);
    p->v1 = c.take<double>(bn);
    p->lrow = c.take<int>(2 * bn);
    p->lsrc = c.take<double>(2 * bn);
    p->pval = c.take<double>(bn * chunks);
    p->parg = c.take<int>(bn * chunks);
    p->inst = c.take<int>((size_t)batch * kOdInstInts);
    s.rowpart = c.take<double>(bn);
    s.gmin = c.take<double>((size_t)batch);
    s.running = c.take<int>(1);
    s.bytes = c.off;
    return s;
}

// Training loss: the column-pass partials, the integer counts the backward reads (K, R, cnt, ksum), the row
// minima of the reduced costs and the hinge partial sums.  The plan fields of *p must be filled.
size_t train_loss_layout(void *ws, TrainLossParams *p)
{
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    const size_t bn = (size_t)p->batch * p->n;
    p->pval = c.take<float>(bn * p->chunks);
    p->parg = c.take<int>(bn * p->chunks);
    p->K = c.take<int>(bn);
    p->R = c.take<int>(bn);
    p->cnt = c.take<int>(bn);
    p->ksum = c.take<int>(bn);
    p->mkey = c.take<unsigned>(bn);
    p->mj = c.take<int>(bn);
    p->hpart = c.take<double>((size_t)p->batch * p->hparts);
    return c.off;
}

// DualGNN loss: the training-loss layout, then d_j and the per-row sums S_i behind it.
size_t dual_loss_layout(void *ws, TrainLossParams *p)
{
    Carver c{reinterpret_cast<unsigned char *>(ws), train_loss_layout(ws, p)};
    const size_t bn = (size_t)p->batch * p->n;
    p->dj = c.take<float>(bn);
    p->vsum = c.take<double>(bn);
    return c.off;
}

// Rectangular / cost-limited lapjv: the extended matrices (none when the solver reads the caller's C),
// the solver's x, y of the n x n problem, the matched costs of the finish step, the cold workspace.
struct ExtendedWs {
    double *E, *gath;
    int *xs, *ys;
    unsigned char *solver;
    size_t solver_bytes, bytes;
};

ExtendedWs extended_layout(void *ws, int batch, int n_rows, int n_cols, int n, bool copy)
{
    ExtendedWs w;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    const size_t bn = (size_t)batch * n;
    w.E = copy ? c.take<double>(bn * n) : nullptr;
    w.xs = c.take<int>(bn);
    w.ys = c.take<int>(bn);
    w.gath = c.take<double>((size_t)batch * n_rows);
    w.solver_bytes = solver_layout(nullptr, batch, n, kModeCold, true).bytes;
    w.solver = c.take<unsigned char>(w.solver_bytes);
    w.bytes = c.off;
    return w;
}

// _lapjv.pyx:84 `cost_limit < np.inf` (false for NaN, as there)
bool cost_limited(double cost_limit) { return cost_limit < (double)INFINITY; }

int device_cus()
{
    static const int cus = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        const bool ok = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess;
        return (ok && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }();
    return cus;
}

// grow-only device arena for the host-pointer entry points
struct Arena {
    std::mutex mu;
    void *ptr = nullptr;
    size_t cap = 0;
    // Lays out the device buffers of one host-pointer call: `layout` takes them from the Carver it is
    // given and returns them.  It runs on a null base to measure the arena, then on the arena itself.
    // All null: the arena could not grow.
    template <typename Layout>
    auto stage(Layout &&layout) -> decltype(layout(std::declval<Carver &>()))
    {
        Carver c{nullptr, 0};
        layout(c);
        if (c.off > cap) {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr;
            cap = 0;
            if (hipMalloc(&ptr, c.off) != hipSuccess) return {};
            cap = c.off;
        }
        c = Carver{reinterpret_cast<unsigned char *>(ptr), 0};
        return layout(c);
    }
};
Arena g_arena;

// optional event bracket around the per-instance solver kernel (bench.py's roofline leg).
// One bracket per process (the benchmark's single submission thread); guarded by g_prof_mu so
// that concurrent callers of the batched entry points cannot corrupt it.
std::mutex g_prof_mu;
bool g_profile = false;
hipEvent_t g_ev0 = nullptr, g_ev1 = nullptr;
bool g_ev_valid = false;

hipError_t profile_begin(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_profile) return hipSuccess;
    if (!g_ev0) {
        hipError_t e = hipEventCreate(&g_ev0);
        if (e != hipSuccess) return e;
        e = hipEventCreate(&g_ev1);
        if (e != hipSuccess) return e;
    }
    return hipEventRecord(g_ev0, s);
}

hipError_t profile_end(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_profile) return hipSuccess;
    g_ev_valid = true;
    return hipEventRecord(g_ev1, s);
}

int check_dims(int batch, int n)
{
    if (n <= 0 || batch <= 0) return -2;
    if (n > kMaxN) return -5;
    return 0;
}

// The prelude of a seeded solve on the prepared u_work, v_work: prelude, projection, prelude again.  `g`: the
// ragged batch (stride n = g->N), or null for a uniform one.  *tight_eps is what the solver is to use.
int seeded_prelude(const double *C, int batch, int n, const PreludeWs &w, double eps, const RaggedBatch *g,
                   hipStream_t stream, double *tight_eps)
{
    PreludeParams pp;
    pp.C = C;
    pp.n = n;
    pp.batch = batch;
    pp.u = w.u_work;
    pp.v = w.v_work;
    pp.eps = eps;
    pp.tight_eps = (eps < 1e-9) ? 1e-9 : eps;  // std::max(eps, 1e-9), lapjv_seeded.cpp:76
    pp.u_tight = w.u_tight;
    pp.viol_cnt = w.viol_cnt;
    pp.tight_cnt = w.tight_cnt;
    pp.tight_bits = w.tight_bits;
    pp.inst_flags = w.flags;
    const auto prelude = [&] { return g ? launch_prelude_ragged(pp, *g, stream) : launch_prelude(pp, stream); };
    pp.rerun = 0;
    HIP_TRY(prelude());
    HIP_TRY(g ? launch_projection_ragged(*g, w.u_work, w.v_work, w.viol_cnt, w.flags, eps, stream)
              : launch_projection(C, n, batch, w.u_work, w.v_work, w.viol_cnt, w.flags, eps, stream));
    pp.rerun = 1;
    HIP_TRY(prelude());
    *tight_eps = pp.tight_eps;
    return 0;
}

// The solves of a ragged batch take no instance the device would treat as empty (size outside 1..N, or wider
// than its row stride).
bool host_sizes_ok(const int *host_sizes, int batch, int N, int ld)
{
    for (int b = 0; b < batch; ++b) {
        if (host_sizes[b] < 1 || host_sizes[b] > N || (ld > 0 && host_sizes[b] > ld)) return false;
    }
    return true;
}

// The kernel argument block of the solver launches of a ragged batch; `pre`: the prelude's buffers of a seeded
// solve (the caller adds tight_eps), null for a cold one.
SolverParams ragged_solver_params(int mode, const RaggedBatch &g, long long *x, long long *y, int *ret,
                                  long long *stats, const PreludeWs *pre)
{
    SolverParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.C = g.C;
    sp.n = g.N;
    sp.batch = g.batch;
    sp.mode = mode;
    if (pre) hand_prelude_to_solver(*pre, &sp);
    sp.x_out = x;
    sp.y_out = y;
    sp.ret = ret;
    sp.stats = stats;
    sp.rg_offsets = g.offsets;
    sp.rg_sizes = g.sizes;
    sp.rg_ld = g.ld;
    sp.rg_N = g.N;
    return sp;
}

// One launch per kernel configuration; the launches are independent and each workgroup picks its own.  The
// bracket of lapwarm_profile_enable holds all solver launches of the call.
int launch_ragged_groups(SolverParams sp, const RaggedGroup *groups, int n_groups, hipStream_t stream)
{
    HIP_TRY(profile_begin(stream));
    for (int k = 0; k < n_groups; ++k) {
        sp.rg_n_lo = groups[k].n_lo;
        sp.rg_n_hi = groups[k].n_hi;
        HIP_TRY(launch_phase_ragged(groups[k].k, sp, stream));
    }
    HIP_TRY(profile_end(stream));
    return 0;
}

// ---- the copies of the host-pointer entry points (blocking, on the null stream) ----
template <typename T>
hipError_t upload(T *dst, const T *src, size_t count)
{
    return hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyHostToDevice);
}

template <typename T>
hipError_t download(T *dst, const T *src, size_t count)
{
    return hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost);
}

// The per-instance code a batch of one left on the device (>= 0), or the code of the copy's failure.
int device_ret(const int *dret)
{
    int ret = 0;
    HIP_TRY(download(&ret, dret, 1));
    return ret;
}

}  // namespace

extern "C" {

const char *lapwarm_last_error(void) { return g_err; }

int lapwarm_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

void lapwarm_profile_enable(int on)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_profile = on != 0;
}

double lapwarm_profile_last_solver_ms(void)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_ev_valid) return -1.0;
    if (hipEventSynchronize(g_ev1) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, g_ev0, g_ev1) != hipSuccess) return -1.0;
    return (double)ms;
}

int lapwarm_refine_aggregate_wsum(const float *topk16, const float *u_pre, const float *w1,
                                  const float *b1, float *out, float *wsum, int rows, int H, void *stream_)
{
    if (rows <= 0 || H <= 0) return -2;
    HIP_TRY(launch_refine_aggregate(topk16, u_pre, w1, b1, out, wsum, rows, H, as_stream(stream_)));
    return 0;
}

int lapwarm_refine_aggregate_batched(const float *topk16, const float *u_pre, const float *w1,
                                     const float *b1, float *out, int rows, int H, int, void *stream_)
{
    return lapwarm_refine_aggregate_wsum(topk16, u_pre, w1, b1, out, nullptr, rows, H, stream_);
}

size_t lapwarm_refine_backward_workspace_bytes(int rows, int H)
{
    return refine_backward_workspace_bytes(rows, H);
}

int lapwarm_refine_backward(const float *topk16, const float *u_pre, const float *w1, const float *b1,
                            const float *grad_out, const float *grad_wsum, float *grad_u, float *grad_w1,
                            float *grad_b1, int rows, int H, void *ws, size_t ws_bytes, void *stream_)
{
    if (rows < 0 || H < 1) return -2;
    if (rows == 0) return 0;
    if (!topk16 || !u_pre || !w1 || !b1 || !grad_out || !grad_u || !grad_w1 || !grad_b1 || !ws) return -2;
    if (ws_bytes < refine_backward_workspace_bytes(rows, H)) return -2;  // (this entry's code: not check_workspace)
    HIP_TRY(launch_refine_backward(topk16, u_pre, w1, b1, grad_out, grad_wsum, grad_u, grad_w1, grad_b1, rows, H, ws,
                                   as_stream(stream_)));
    return 0;
}

size_t lapwarm_graph_features_workspace_bytes(int batch, int n) { return graph_features_workspace_bytes(batch, n); }

int lapwarm_graph_features_batched(const double *C, int batch, int n, const double *u, const float *posenc,
                                   float *edge_out, float *row_out, float *col_out, void *ws, size_t ws_bytes,
                                   void *stream_)
{
    if (batch < 1 || batch > kGraphMaxBatch || n < 1) return -2;
    if (n > kGraphMaxN) return -5;
    if (!C || !posenc || !edge_out || !row_out || !col_out || !ws) return -2;
    if (int rc = check_workspace(ws_bytes, graph_features_workspace_bytes(batch, n))) return rc;
    GraphFeatureParams p{C, u, posenc, batch, n, edge_out, row_out, col_out};
    HIP_TRY(launch_graph_features(p, ws, as_stream(stream_)));
    return 0;
}

size_t lapwarm_dual_gnn_workspace_bytes(int batch, int n, int heads) { return dual_gnn_workspace_bytes(batch, n, heads); }

// The checks of the four edge-score forwards, in the order the ABI keeps: dimensions (heads by kDualMaxHeads, the
// kernel's tile limit), n, pointers.  An entry that takes p checks it before it comes here.
static bool dual_edge_null(const DualEdgeParams &p)
{
    return !p.edge_feat || !p.W1 || !p.b1 || !p.W2 || !p.b2 || !p.G;
}

static int dual_edge_scores(const DualEdgeParams &p, float *scores, bool need_sizes, void *stream_)
{
    if (p.batch < 1 || p.batch > kDualMaxBatch || p.n < 1 || p.heads < 1 || p.heads > kDualMaxHeads) return -2;
    if (p.n > kMaxN) return -5;
    if (dual_edge_null(p) || !scores || (need_sizes && !p.sizes)) return -2;
    HIP_TRY(launch_dual_edge_scores(p, scores, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_edge_scores(const float *edge_feat, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *G, float *scores, int batch, int n, int heads, void *stream_)
{
    return dual_edge_scores({edge_feat, W1, b1, W2, b2, G, nullptr, batch, n, heads}, scores, false, stream_);
}

// The checks of the five attention forwards.  heads: the grid's y dimension, not kDualMaxHeads.
static int dual_attention(const DualAttnParams &p, bool need_stats, bool need_sizes, void *stream_)
{
    if (p.batch < 1 || p.batch > kDualMaxBatch || p.n < 1 || p.heads < 1 || p.heads > kMaxGridY || p.head_dim < 1)
        return -2;
    if (p.n > kMaxN) return -5;
    if (!p.scores || !p.a_row || !p.c_row || !p.a_col || !p.c_col || !p.kbias || !p.row_val || !p.col_val ||
        !p.row_msg || !p.col_msg || (need_stats && (!p.row_stats || !p.col_stats)) || (need_sizes && !p.sizes))
        return -2;
    HIP_TRY(launch_dual_attention(p, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_attention(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                           const float *c_col, const float *kbias, const unsigned char *mask, const float *row_val,
                           const float *col_val, float *row_msg, float *col_msg, int batch, int n, int heads,
                           int head_dim, void *stream_)
{
    DualAttnParams p{scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val, row_msg, col_msg,
                     batch, n, heads, head_dim};
    return dual_attention(p, false, false, stream_);
}

// ---- DualGNN on a ragged batch: the features (graph_features.hip) and the size-aware attention (dual_gnn.hip) ----
size_t lapwarm_graph_features_ragged_workspace_bytes(int batch, int N)
{
    return graph_features_ragged_workspace_bytes(batch, N);
}

int lapwarm_graph_features_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                  const double *u, const float *posenc, const int *pos_off, float *edge_out,
                                  float *row_out, float *col_out, unsigned char *mask, int *ret, void *ws,
                                  size_t ws_bytes, void *stream_)
{
    if (batch < 1 || batch > kGraphMaxBatch || N < 1 || ld < 0) return -2;
    if (N > kGraphMaxN) return -5;
    if (!C || !offsets || !sizes || !posenc || !pos_off || !edge_out || !row_out || !col_out || !mask || !ret || !ws)
        return -2;
    if (int rc = check_workspace(ws_bytes, graph_features_ragged_workspace_bytes(batch, N))) return rc;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    const GraphFeatureRaggedOut o{u, posenc, pos_off, edge_out, row_out, col_out, mask, ret};
    HIP_TRY(launch_graph_features_ragged(g, o, ws, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_edge_scores_ragged(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                    const float *b2, const float *G, float *scores, const int *sizes, int batch, int n,
                                    int heads, void *stream_)
{
    return dual_edge_scores({edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads}, scores, true, stream_);
}

int lapwarm_dual_attention_ragged(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                  const float *c_col, const float *kbias, const int *sizes, const float *row_val,
                                  const float *col_val, float *row_msg, float *col_msg, int batch, int n, int heads,
                                  int head_dim, void *stream_)
{
    DualAttnParams p{scores, a_row, c_row, a_col, c_col, kbias, nullptr, row_val, col_val, row_msg, col_msg,
                     batch, n, heads, head_dim, sizes};
    return dual_attention(p, false, true, stream_);
}

// ---- DualGNN training: the forward with its softmax statistics, and the two backwards (dual_gnn.hip) ----
int lapwarm_dual_attention_stats(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                 const float *c_col, const float *kbias, const unsigned char *mask,
                                 const float *row_val, const float *col_val, float *row_msg, float *col_msg,
                                 float *row_stats, float *col_stats, int batch, int n, int heads, int head_dim,
                                 void *stream_)
{
    DualAttnParams p{scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val, row_msg, col_msg,
                     batch, n, heads, head_dim, nullptr, row_stats, col_stats};
    return dual_attention(p, true, false, stream_);
}

int lapwarm_dual_attention_stats_ragged(const float *scores, const float *a_row, const float *c_row,
                                        const float *a_col, const float *c_col, const float *kbias, const int *sizes,
                                        const float *row_val, const float *col_val, float *row_msg, float *col_msg,
                                        float *row_stats, float *col_stats, int batch, int n, int heads, int head_dim,
                                        void *stream_)
{
    if (!sizes) return -2;  // before the dimensions here: n > kMaxN with null sizes is -2
    DualAttnParams p{scores, a_row, c_row, a_col, c_col, kbias, nullptr, row_val, col_val, row_msg, col_msg,
                     batch, n, heads, head_dim, sizes, row_stats, col_stats};
    return dual_attention(p, true, true, stream_);
}

size_t lapwarm_dual_backward_workspace_bytes(int batch, int n, int heads)
{
    return dual_backward_workspace_bytes(batch, n, heads);
}

int lapwarm_dual_backward_chunk(void) { return kDualBwdChunk; }

// p in [0, 1), before any HIP call and before every other check of an entry that takes p; p == 0 leaves `on` false,
// which selects the kernels without the generator, and the record DualDropout{}
static int dual_dropout_of(unsigned long long seed, double p, DualDropout *d)
{
    if (!(p >= 0.0 && p < 1.0)) return -2;  // NaN included
    d->k0 = (unsigned)seed;
    d->k1 = (unsigned)(seed >> 32);
    d->threshold = (unsigned)(p * 4294967296.0);  // floor(p 2^32) <= 2^32 - 1
    d->scale = (float)(1.0 / (1.0 - p));
    d->on = p > 0.0;
    return 0;
}

// Both backwards bound heads by kDualMaxHeads (the workspace's limit) and check the workspace last.
static int dual_attention_backward(DualAttnBwdParams p, void *workspace, size_t workspace_bytes, void *stream_)
{
    const DualAttnParams &f = p.fwd;
    if (f.batch < 1 || f.batch > kDualMaxBatch || f.n < 1 || f.heads < 1 || f.heads > kDualMaxHeads || f.head_dim < 1)
        return -2;
    if (f.n > kMaxN) return -5;
    if (!f.scores || !f.a_row || !f.c_row || !f.a_col || !f.c_col || !f.kbias || !f.row_val || !f.col_val ||
        !f.row_msg || !f.col_msg || !f.row_stats || !f.col_stats || !p.d_row_msg || !p.d_col_msg || !p.dS ||
        !p.da_row || !p.dc_row || !p.da_col || !p.dc_col || !p.dkb || !p.d_row_val || !p.d_col_val || !workspace)
        return -2;
    if (int rc = check_workspace(workspace_bytes, dual_backward_workspace_bytes(f.batch, f.n, f.heads))) return rc;
    p.partials = static_cast<double *>(workspace);
    HIP_TRY(launch_dual_attention_backward(p, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_attention_backward_dropout(const float *scores, const float *a_row, const float *c_row,
                                            const float *a_col, const float *c_col, const float *kbias,
                                            const unsigned char *mask, const int *sizes, const float *row_val,
                                            const float *col_val, const float *row_msg, const float *col_msg,
                                            const float *row_stats, const float *col_stats, const float *d_row_msg,
                                            const float *d_col_msg, float *dS, float *da_row, float *dc_row,
                                            float *da_col, float *dc_col, float *dkb, float *d_row_val,
                                            float *d_col_val, int batch, int n, int heads, int head_dim,
                                            void *workspace, size_t workspace_bytes, unsigned long long seed, double p,
                                            void *stream_)
{
    DualAttnBwdParams q{{scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val,
                         const_cast<float *>(row_msg), const_cast<float *>(col_msg), batch, n, heads, head_dim, sizes,
                         const_cast<float *>(row_stats), const_cast<float *>(col_stats)},
                        d_row_msg, d_col_msg, dS, da_row, dc_row, da_col, dc_col, dkb, d_row_val, d_col_val, nullptr};
    if (int rc = dual_dropout_of(seed, p, &q.fwd.drop)) return rc;
    return dual_attention_backward(q, workspace, workspace_bytes, stream_);
}

int lapwarm_dual_attention_backward(const float *scores, const float *a_row, const float *c_row, const float *a_col,
                                    const float *c_col, const float *kbias, const unsigned char *mask,
                                    const int *sizes, const float *row_val, const float *col_val,
                                    const float *row_msg, const float *col_msg, const float *row_stats,
                                    const float *col_stats, const float *d_row_msg, const float *d_col_msg, float *dS,
                                    float *da_row, float *dc_row, float *da_col, float *dc_col, float *dkb,
                                    float *d_row_val, float *d_col_val, int batch, int n, int heads, int head_dim,
                                    void *workspace, size_t workspace_bytes, void *stream_)
{
    // seed 0, p 0: no dropout
    return lapwarm_dual_attention_backward_dropout(scores, a_row, c_row, a_col, c_col, kbias, mask, sizes, row_val,
                                                   col_val, row_msg, col_msg, row_stats, col_stats, d_row_msg,
                                                   d_col_msg, dS, da_row, dc_row, da_col, dc_col, dkb, d_row_val,
                                                   d_col_val, batch, n, heads, head_dim, workspace, workspace_bytes, 0,
                                                   0.0, stream_);
}

static int dual_edge_scores_backward(const DualEdgeParams &p, const float *dS, const DualEdgeGrads &g, void *workspace,
                                     size_t workspace_bytes, void *stream_)
{
    if (p.batch < 1 || p.batch > kDualMaxBatch || p.n < 1 || p.heads < 1 || p.heads > kDualMaxHeads) return -2;
    if (p.n > kMaxN) return -5;
    if (dual_edge_null(p) || !dS || !g.dW1 || !g.db1 || !g.dW2 || !g.db2 || !g.dG || !workspace) return -2;
    if (int rc = check_workspace(workspace_bytes, dual_backward_workspace_bytes(p.batch, p.n, p.heads))) return rc;
    HIP_TRY(launch_dual_edge_scores_backward(p, dS, g, workspace, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_edge_scores_backward(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                      const float *b2, const float *G, const float *dS, const int *sizes, float *dW1,
                                      float *db1, float *dW2, float *db2, float *dG, int batch, int n, int heads,
                                      void *workspace, size_t workspace_bytes, void *stream_)
{
    return dual_edge_scores_backward({edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads}, dS,
                                     {dW1, db1, dW2, db2, dG}, workspace, workspace_bytes, stream_);
}

// ---- DualGNN training with the two dropouts of the fused region (dual_dropout.hpp); sizes nullable ----
int lapwarm_dual_edge_scores_dropout(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                     const float *b2, const float *G, float *scores, const int *sizes, int batch, int n,
                                     int heads, unsigned long long seed, double p, void *stream_)
{
    DualEdgeParams q{edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads};
    if (int rc = dual_dropout_of(seed, p, &q.drop)) return rc;
    return dual_edge_scores(q, scores, false, stream_);
}

int lapwarm_dual_attention_stats_dropout(const float *scores, const float *a_row, const float *c_row,
                                         const float *a_col, const float *c_col, const float *kbias,
                                         const unsigned char *mask, const int *sizes, const float *row_val,
                                         const float *col_val, float *row_msg, float *col_msg, float *row_stats,
                                         float *col_stats, int batch, int n, int heads, int head_dim,
                                         unsigned long long seed, double p, void *stream_)
{
    DualAttnParams q{scores, a_row, c_row, a_col, c_col, kbias, mask, row_val, col_val, row_msg, col_msg,
                     batch, n, heads, head_dim, sizes, row_stats, col_stats};
    if (int rc = dual_dropout_of(seed, p, &q.drop)) return rc;
    return dual_attention(q, true, false, stream_);
}

int lapwarm_dual_edge_scores_backward_dropout(const float *edge_feat, const float *W1, const float *b1,
                                              const float *W2, const float *b2, const float *G, const float *dS,
                                              const int *sizes, float *dW1, float *db1, float *dW2, float *db2,
                                              float *dG, int batch, int n, int heads, void *workspace,
                                              size_t workspace_bytes, unsigned long long seed, double p, void *stream_)
{
    DualEdgeParams q{edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads};
    if (int rc = dual_dropout_of(seed, p, &q.drop)) return rc;
    return dual_edge_scores_backward(q, dS, {dW1, db1, dW2, db2, dG}, workspace, workspace_bytes, stream_);
}

// ---- the edge MLP on the bf16 MFMA units (dual_gnn.hip); sizes nullable, p == 0: no dropout ----
int lapwarm_dual_edge_scores_bf16(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                  const float *b2, const float *G, float *scores, const int *sizes, int batch, int n,
                                  int heads, unsigned long long seed, double p, void *stream_)
{
    DualEdgeParams q{edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads};
    if (int rc = dual_dropout_of(seed, p, &q.drop)) return rc;
    q.bf16 = true;
    return dual_edge_scores(q, scores, false, stream_);
}

int lapwarm_dual_edge_scores_backward_bf16(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                           const float *b2, const float *G, const float *dS, const int *sizes,
                                           float *dW1, float *db1, float *dW2, float *db2, float *dG, int batch, int n,
                                           int heads, void *workspace, size_t workspace_bytes, unsigned long long seed,
                                           double p, void *stream_)
{
    DualEdgeParams q{edge_feat, W1, b1, W2, b2, G, sizes, batch, n, heads};
    if (int rc = dual_dropout_of(seed, p, &q.drop)) return rc;
    q.bf16 = true;
    return dual_edge_scores_backward(q, dS, {dW1, db1, dW2, db2, dG}, workspace, workspace_bytes, stream_);
}


int lapwarm_dual_dropout_keep(unsigned long long seed, unsigned int stream_id, unsigned long long first,
                              unsigned long long count, double p, unsigned char *keep, void *stream_)
{
    DualDropout drop;
    if (int rc = dual_dropout_of(seed, p, &drop)) return rc;
    if (count == 0) return 0;
    if (!keep || count >= (1ull << 39)) return -2;  // the grid's x dimension: 2^31 blocks of 256
    HIP_TRY(launch_dual_dropout_keep(drop, stream_id, first, count, keep, as_stream(stream_)));
    return 0;
}

int lapwarm_solver_uses_helpers(int n)
{
    return (solver_uses_helpers(n) && solve_shape(n, false) == SolveShape::kOneLaunch) ? 1 : 0;
}

int lapwarm_coop_members(int n) { return n > 0 ? coop_config(n).members : 0; }

const char *lapwarm_build_info(void) { return "liblapwarm_hip gfx950 (hand-written HIP, fp64)"; }

size_t lapwarm_seeded_workspace_bytes(int batch, int n)
{
    if (check_dims(batch, n)) return 0;
    return solver_layout(nullptr, batch, n, kModeSeeded, false).bytes;
}

size_t lapwarm_lapjv_workspace_bytes(int batch, int n)
{
    if (check_dims(batch, n)) return 0;
    return solver_layout(nullptr, batch, n, kModeCold, true).bytes;
}

size_t lapwarm_sweep_workspace_bytes(int batch, int n)
{
    if (check_dims(batch, n)) return 0;
    return sweep_layout(nullptr, batch, n).bytes;
}

int lapwarm_seeded_batched(const double *C, int batch, int n, const double *u_seed,
                           const double *v_seed, double eps, long long *x, long long *y, int *ret,
                           long long *stats, void *workspace, size_t workspace_bytes,
                           int threads_hint, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    hipStream_t stream = as_stream(stream_);
    SolverWs w = solver_layout(workspace, batch, n, kModeSeeded, false);
    SolverParams &sp = w.sp;
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    HIP_TRY(launch_seed_prepare(u_seed, v_seed, w.pre.u_work, w.pre.v_work, (size_t)batch * n, w.pre.flags, batch,
                                sp.pf_ring, batch * kRingInts, stream));
    if (int rc = seeded_prelude(C, batch, n, w.pre, eps, nullptr, stream, &sp.tight_eps)) return rc;
    sp.C = C;
    sp.x_out = x;
    sp.y_out = y;
    sp.ret = ret;
    sp.stats = stats;
    HIP_TRY(profile_begin(stream));
    HIP_TRY(launch_solver(plan_solve(kModeSeeded, batch, n, threads_hint, w.lists, device_cus()), sp, stream));
    HIP_TRY(profile_end(stream));
    return 0;
}

static int lapjv_batched_impl(const double *C, int batch, int n, int *x, int *y, double *u, double *v,
                              int *ret, long long *stats, void *workspace, size_t workspace_bytes,
                              int threads_hint, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    hipStream_t stream = as_stream(stream_);
    // a workspace of lapwarm_lapjv_workspace_bytes() carries the candidate lists of the row reduction;
    // the smaller lapwarm_seeded_workspace_bytes() is still accepted (plain row scans then)
    SolverWs w = solver_layout(workspace, batch, n, kModeCold, true);
    if (workspace_bytes < w.bytes) w = solver_layout(workspace, batch, n, kModeCold, false);
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    SolverParams &sp = w.sp;
    sp.C = C;
    sp.x32_out = x;
    sp.y32_out = y;
    sp.v_out = v;
    sp.u_out = u;
    sp.ret = ret;
    sp.stats = stats;
    HIP_TRY(profile_begin(stream));
    HIP_TRY(launch_solver(plan_solve(kModeCold, batch, n, threads_hint, w.lists, device_cus()), sp, stream));
    HIP_TRY(profile_end(stream));
    return 0;
}

int lapwarm_lapjv_batched(const double *C, int batch, int n, int *x, int *y, int *ret,
                          long long *stats, void *workspace, size_t workspace_bytes,
                          int threads_hint, void *stream_)
{
    return lapjv_batched_impl(C, batch, n, x, y, nullptr, nullptr, ret, stats, workspace, workspace_bytes,
                              threads_hint, stream_);
}

int lapwarm_lapjv_duals_batched(const double *C, int batch, int n, int *x, int *y, double *u, double *v,
                                int *ret, long long *stats, void *workspace, size_t workspace_bytes,
                                int threads_hint, void *stream_)
{
    return lapjv_batched_impl(C, batch, n, x, y, u, v, ret, stats, workspace, workspace_bytes, threads_hint,
                              stream_);
}

int lapwarm_lapjv_extended_n(int n_rows, int n_cols, int extend_cost, double cost_limit)
{
    if (n_rows <= 0 || n_cols <= 0) return -2;
    if (n_rows != n_cols && !extend_cost) return -4;  // _lapjv.pyx:80-83, whatever the limit
    const long long n = cost_limited(cost_limit) ? (long long)n_rows + n_cols
                                                 : (n_rows > n_cols ? n_rows : n_cols);
    return n > kMaxN ? -5 : (int)n;
}

size_t lapwarm_lapjv_extended_workspace_bytes(int batch, int n_rows, int n_cols, int extend_cost,
                                              double cost_limit)
{
    const int n = lapwarm_lapjv_extended_n(n_rows, n_cols, extend_cost, cost_limit);
    if (n <= 0 || batch <= 0) return 0;
    const bool copy = cost_limited(cost_limit) || n_rows != n_cols;
    return extended_layout(nullptr, batch, n_rows, n_cols, n, copy).bytes;
}

int lapwarm_lapjv_extended_batched(const double *C, int batch, int n_rows, int n_cols, int extend_cost,
                                   double cost_limit, int *x, int *y, double *opt, int *matched, int *ret,
                                   long long *stats, void *workspace, size_t workspace_bytes,
                                   int threads_hint, void *stream_)
{
    const int n = lapwarm_lapjv_extended_n(n_rows, n_cols, extend_cost, cost_limit);
    if (n < 0) return n;
    if (batch <= 0 || batch > kMaxGridY) return -2;  // (the extension kernel's grid: rows x batch)
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return -2;  // E is written with 16-byte stores
    hipStream_t stream = as_stream(stream_);
    const bool limited = cost_limited(cost_limit);
    // a square matrix without a limit is solved where it is (_lapjv.pyx:91-95 copies it into zeros)
    const bool copy = limited || n_rows != n_cols;
    const ExtendedWs w = extended_layout(workspace, batch, n_rows, n_cols, n, copy);
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    if (copy)
        HIP_TRY(launch_extend_costs(C, batch, n_rows, n_cols, n, limited ? cost_limit / 2. : 0.0, w.E, stream));
    if (int rc = lapjv_batched_impl(copy ? w.E : C, batch, n, w.xs, w.ys, nullptr, nullptr, ret, stats, w.solver,
                                    w.solver_bytes, threads_hint, stream_))
        return rc;
    HIP_TRY(launch_extended_finish(C, batch, n_rows, n_cols, n, w.xs, w.ys, ret, x, y, opt, matched, w.gath,
                                   stream));
    return 0;
}

int lapwarm_colmin_batched(const double *C, int batch, int n, const double *u, double *out,
                           void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (int rc = check_workspace(workspace_bytes, lapwarm_sweep_workspace_bytes(batch, n))) return rc;
    HIP_TRY(launch_colmin(C, n, batch, u, out, sweep_layout(workspace, batch, n).partial, as_stream(stream_)));
    return 0;
}

int lapwarm_rowmin_batched(const double *C, int batch, int n, const double *v, double *out, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    HIP_TRY(launch_rowmin(C, n, batch, v, out, as_stream(stream_)));
    return 0;
}

int lapwarm_row_features_batched(const double *C, int batch, int n, const float *posenc, float *feat,
                                 float *topk16, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (int rc = check_workspace(workspace_bytes, lapwarm_sweep_workspace_bytes(batch, n))) return rc;
    hipStream_t stream = as_stream(stream_);
    const SweepWs w = sweep_layout(workspace, batch, n);
    HIP_TRY(launch_colmin(C, n, batch, nullptr, w.colmin, w.partial, stream));
    FeatureParams fp;
    fp.C = C;
    fp.n = n;
    fp.batch = batch;
    fp.colmin = w.colmin;
    fp.posenc = posenc;
    fp.feat = feat;
    fp.topk = topk16;
    HIP_TRY(launch_row_features(fp, stream));
    return 0;
}

// ---- ragged batches: B instances of different sizes behind one offset and one size per instance ----
static int check_ragged(const void *C, const void *offsets, const void *sizes, int ld, int batch, int N)
{
    const int rc = check_ragged_dims(batch, N);
    if (rc == -2 || ld < 0) return -2;
    if (rc) return rc;
    if (!C || !offsets || !sizes) return -2;
    return 0;
}

size_t lapwarm_ragged_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return align_up(sizeof(double) * (size_t)batch * N);  // the column minima the feature kernel compares with
}

int lapwarm_colmin_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                          const double *u, double *out, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!out || !workspace) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_ragged_workspace_bytes(batch, N))) return rc;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    HIP_TRY(launch_colmin_ragged(g, u, out, as_stream(stream_)));
    return 0;
}

int lapwarm_row_features_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                const float *posenc, const int *pos_off, float *feat, float *topk16, float *cost32,
                                unsigned char *mask, int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!posenc || !pos_off || !feat || !ret || !workspace) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_ragged_workspace_bytes(batch, N))) return rc;
    hipStream_t stream = as_stream(stream_);
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    double *colmin = reinterpret_cast<double *>(workspace);
    HIP_TRY(launch_colmin_ragged(g, nullptr, colmin, stream));
    const RaggedFeatureOut o{colmin, posenc, pos_off, feat, topk16, cost32, mask, ret};
    HIP_TRY(launch_row_features_ragged(g, o, stream));
    return 0;
}

size_t lapwarm_seeded_ragged_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return ragged_solver_layout(nullptr, batch, N).bytes;
}

int lapwarm_seeded_ragged_groups(const int *sizes, int batch, int *group_of)
{
    if (!sizes || !group_of || batch <= 0) return -2;
    RaggedGroup groups[kMaxRaggedGroups];
    return plan_ragged_groups(sizes, batch, group_of, groups);
}

int lapwarm_seeded_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes, int ld,
                          int batch, int N, const double *u_seed, const double *v_seed, double eps, long long *x,
                          long long *y, int *ret, long long *stats, void *workspace, size_t workspace_bytes,
                          void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!host_sizes || !u_seed || !v_seed || !x || !y || !ret || !workspace) return -2;
    if (!host_sizes_ok(host_sizes, batch, N, ld)) return -2;
    RaggedGroup groups[kMaxRaggedGroups];
    const int n_groups = plan_ragged_groups(host_sizes, batch, nullptr, groups);
    if (n_groups < 0) {
        snprintf(g_err, sizeof(g_err), "lapwarm_seeded_ragged: an instance is outside the one-launch, all-LDS class");
        return -6;
    }
    const RaggedSolverWs w = ragged_solver_layout(workspace, batch, N);
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    const PreludeWs &pre = w.pre;
    hipStream_t stream = as_stream(stream_);
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    HIP_TRY(launch_seed_prepare_ragged(g, u_seed, v_seed, pre.u_work, pre.v_work, pre.flags, x, y, ret, stats,
                                       stream));
    SolverParams sp = ragged_solver_params(kModeSeeded, g, x, y, ret, stats, &pre);
    if (int rc = seeded_prelude(C, batch, N, pre, eps, &g, stream, &sp.tight_eps)) return rc;
    return launch_ragged_groups(sp, groups, n_groups, stream);
}

// ---- cold lapjv of a ragged batch (extend_ragged.hip around the ragged launches of jv_instance_kernel) ----
size_t lapwarm_lapjv_ragged_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return align_up(1);  // every eligible instance keeps its solver state in LDS: the workspace is not used
}

int lapwarm_lapjv_ragged_groups(const int *sizes, int batch, int *group_of)
{
    if (!sizes || !group_of || batch <= 0) return -2;
    RaggedGroup groups[kMaxRaggedGroups];
    return plan_ragged_groups_cold(sizes, batch, group_of, groups);
}

int lapwarm_lapjv_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes, int ld,
                         int batch, int N, long long *x, long long *y, int *ret, long long *stats, void *workspace,
                         size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!host_sizes || !x || !y || !ret || !workspace) return -2;
    if (!host_sizes_ok(host_sizes, batch, N, ld)) return -2;
    RaggedGroup groups[kMaxRaggedGroups];
    const int n_groups = plan_ragged_groups_cold(host_sizes, batch, nullptr, groups);
    if (n_groups < 0) {
        snprintf(g_err, sizeof(g_err), "lapwarm_lapjv_ragged: an instance is outside the one-launch, all-LDS, no-lists class");
        return -6;
    }
    if (int rc = check_workspace(workspace_bytes, lapwarm_lapjv_ragged_workspace_bytes(batch, N))) return rc;
    hipStream_t stream = as_stream(stream_);
    HIP_TRY(launch_lapjv_ragged_init(x, y, ret, stats, batch, N, stream));
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    return launch_ragged_groups(ragged_solver_params(kModeCold, g, x, y, ret, stats, nullptr), groups, n_groups,
                                stream);
}

// Rectangular / cost-limited lapjv of a ragged batch: the shapes block (E offsets and extended sizes), the
// solver's x, y [batch][N] int64, the matched costs [batch][R], then the packed E_b: sum of n_b^2 elements.
struct ExtendedRaggedWs {
    long long *e_off, *xs, *ys;
    int *e_n;
    double *gath, *E;
    size_t bytes;
};

static ExtendedRaggedWs extended_ragged_layout(void *ws, int batch, int N, int R, long long e_total)
{
    ExtendedRaggedWs w;
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    w.e_off = c.take<long long>((size_t)batch);
    w.e_n = c.take<int>((size_t)batch);
    w.xs = c.take<long long>((size_t)batch * N);
    w.ys = c.take<long long>((size_t)batch * N);
    w.gath = c.take<double>((size_t)batch * R);
    w.E = c.take<double>((size_t)e_total);
    w.bytes = c.off;
    return w;
}

// The host's plan of a ragged extended call: sizes [batch] = n_b, their largest, the sum of their squares and the
// largest n_rows.  Returns 0 or the argument code (-2, -4, -5) of the first instance that has one.
static int extended_ragged_sizes(const int *host_rows, const int *host_cols, const double *host_limits,
                                 int extend_cost, int batch, std::vector<int> *sizes, int *N, int *R, int *Q,
                                 long long *e_total)
{
    if (batch <= 0 || batch > kMaxGridY || !host_rows || !host_cols || !host_limits) return -2;
    sizes->resize((size_t)batch);
    *N = *R = *Q = 0;
    *e_total = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = lapwarm_lapjv_extended_n(host_rows[b], host_cols[b], extend_cost, host_limits[b]);
        if (n < 0) return n;
        (*sizes)[b] = n;
        if (n > *N) *N = n;
        if (host_rows[b] > *R) *R = host_rows[b];
        if (host_cols[b] > *Q) *Q = host_cols[b];
        *e_total += (long long)n * n;
    }
    return 0;
}

size_t lapwarm_lapjv_extended_ragged_workspace_bytes(const int *host_rows, const int *host_cols,
                                                     const double *host_limits, int extend_cost, int batch)
{
    std::vector<int> sizes;
    int N, R, Q;
    long long e_total;
    if (extended_ragged_sizes(host_rows, host_cols, host_limits, extend_cost, batch, &sizes, &N, &R, &Q, &e_total))
        return 0;
    return extended_ragged_layout(nullptr, batch, N, R, e_total).bytes;
}

int lapwarm_lapjv_extended_ragged(const double *C, const long long *offsets, const int *n_rows, const int *n_cols,
                                  const double *cost_limit, const int *host_rows, const int *host_cols,
                                  const double *host_limits, int ld, int extend_cost, int batch, int R, int Q, int *x,
                                  int *y, double *opt, int *matched, int *ret, long long *stats, void *workspace,
                                  size_t workspace_bytes, void *stream_)
{
    std::vector<int> sizes;
    int N, Rmax, Qmax;
    long long e_total;
    if (int rc = extended_ragged_sizes(host_rows, host_cols, host_limits, extend_cost, batch, &sizes, &N, &Rmax, &Qmax,
                                       &e_total))
        return rc;
    if (ld < 0 || R < Rmax || Q < Qmax || (ld > 0 && Qmax > ld)) return -2;
    if (!C || !offsets || !n_rows || !n_cols || !cost_limit || !x || !y || !ret || !workspace) return -2;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return -2;  // E is written with 16-byte stores
    RaggedGroup groups[kMaxRaggedGroups];
    const int n_groups = plan_ragged_groups_cold(sizes.data(), batch, nullptr, groups);
    if (n_groups < 0) {
        snprintf(g_err, sizeof(g_err),
                 "lapwarm_lapjv_extended_ragged: an instance is outside the one-launch, all-LDS, no-lists class");
        return -6;
    }
    const ExtendedRaggedWs w = extended_ragged_layout(workspace, batch, N, R, e_total);
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    hipStream_t stream = as_stream(stream_);
    const ExtRagged g{C, offsets, n_rows, n_cols, cost_limit, ld, extend_cost ? 1 : 0, batch, R, Q, N, e_total,
                      w.e_off, w.e_n, w.E};
    HIP_TRY(launch_extend_shapes(g, stream));
    HIP_TRY(launch_extend_costs_ragged(g, ret, stats, stream));
    const RaggedBatch extended{w.E, w.e_off, w.e_n, 0, batch, N};
    if (int rc = launch_ragged_groups(ragged_solver_params(kModeCold, extended, w.xs, w.ys, ret, stats, nullptr),
                                      groups, n_groups, stream))
        return rc;
    HIP_TRY(launch_extended_finish_ragged(g, w.xs, w.ys, ret, x, y, opt, matched, w.gath, stream));
    return 0;
}

// ---- sparse LAPMOD of a batch of CSR problems (lapmod_sparse.hip) ----
// Workspace: the state offsets [batch], then the state of every instance above the LDS bound, one behind the other.
struct LapmodWs {
    long long *ws_off;
    unsigned char *state;
    size_t state_bytes, bytes;
    int lds_n;  // the largest host size that keeps its state in LDS
    bool any_global;
};

static int lapmod_layout(void *ws, const int *host_sizes, const long long *host_nnz, int batch, int N, LapmodWs *w)
{
    if (batch <= 0 || batch > kMaxGridY || !host_sizes) return -2;
    const int lds_max = lapmod_lds_max_n();
    size_t state = 0;
    w->lds_n = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = host_sizes[b];
        if (n < 1 || (N > 0 && n > N)) return -2;
        if (n > kLapmodMaxN) return -5;
        if (host_nnz && (host_nnz[b] < 0 || host_nnz[b] > (long long)n * n)) return -2;
        if (n <= lds_max) {
            if (n > w->lds_n) w->lds_n = n;
        } else {
            state += lapmod_state_bytes(n);
        }
    }
    Carver c{reinterpret_cast<unsigned char *>(ws), 0};
    w->ws_off = c.take<long long>((size_t)batch);
    w->state = c.take<unsigned char>(state);
    w->state_bytes = state;
    w->any_global = state > 0;
    w->bytes = c.off;
    return 0;
}

size_t lapwarm_lapmod_workspace_bytes(const int *sizes, const long long *nnz, int batch)
{
    LapmodWs w;
    if (lapmod_layout(nullptr, sizes, nnz, batch, 0, &w)) return 0;
    return w.bytes;
}

int lapwarm_lapmod_lds_max_n(void) { return lapmod_lds_max_n(); }

int lapwarm_lapmod_ragged(const double *cc, const int *kk, const int *ii, const long long *nnz_offsets,
                          const long long *row_offsets, const int *sizes, const int *host_sizes, int batch, int N,
                          int fp_version, int *x, int *y, double *v, int *ret, long long *stats, void *workspace,
                          size_t workspace_bytes, void *stream_)
{
    if (N <= 0 || fp_version < 1 || fp_version > 3) return -2;
    if (N > kLapmodMaxN) return -5;
    LapmodWs w;
    if (int rc = lapmod_layout(workspace, host_sizes, nullptr, batch, N, &w)) return rc;
    if (!cc || !kk || !ii || !nnz_offsets || !row_offsets || !sizes || !x || !y || !ret || !workspace) return -2;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return -2;
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    hipStream_t stream = as_stream(stream_);
    LapmodParams p;
    p.cc = cc;
    p.kk = kk;
    p.ii = ii;
    p.nnz_off = nnz_offsets;
    p.row_off = row_offsets;
    p.sizes = sizes;
    p.batch = batch;
    p.N = N;
    p.fp_version = fp_version;
    p.lds_n = w.lds_n;
    p.x = x;
    p.y = y;
    p.v = v;
    p.ret = ret;
    p.stats = stats;
    p.ws_off = w.any_global ? w.ws_off : nullptr;
    p.ws_state = w.state;
    p.ws_state_bytes = w.state_bytes;
    if (w.any_global) HIP_TRY(launch_lapmod_plan(p, stream));
    HIP_TRY(launch_lapmod(p, stream));
    return 0;
}

// ---- pruning and pricing of dense rows into CSR (prune_price.hip) ----
static PruneWs prune_layout(void *workspace, int batch, int N)
{
    Carver c{reinterpret_cast<unsigned char *>(workspace), 0};
    const size_t bn = (size_t)batch * N;
    PruneWs w;
    w.thr = c.take<unsigned long long>(bn);
    w.ties = c.take<int>(bn);
    w.len = c.take<int>(bn);
    w.nelig = c.take<int>(bn);
    w.bad = c.take<int>(bn);
    w.bytes = c.off;
    return w;
}

size_t lapwarm_prune_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return prune_layout(nullptr, batch, N).bytes;
}

int lapwarm_prune_grow_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                              const double *key, const int *x, const int *kk_in, const int *ii_in,
                              const long long *nnz_offsets_in, const long long *row_offsets_in, int m, double *cc_out,
                              int *kk_out, int *ii_out, const long long *nnz_offsets_out,
                              const long long *row_offsets_out, const long long *cap_out, long long *added,
                              long long *viol, int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (m < 1 || m > kPruneMaxM || !added || !viol || !ret || !workspace) return -2;
    if (x && !key) return -2;
    if (kk_in ? (!ii_in || !nnz_offsets_in || !row_offsets_in) : (ii_in || nnz_offsets_in || row_offsets_in)) return -2;
    if (cc_out ? (!kk_out || !ii_out || !nnz_offsets_out || !row_offsets_out || !cap_out)
               : (kk_out || ii_out || nnz_offsets_out || row_offsets_out || cap_out))
        return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_prune_workspace_bytes(batch, N))) return rc;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    const PruneGrow p{key,    x,      kk_in,  ii_in,           nnz_offsets_in,  row_offsets_in, m,     cc_out,
                      kk_out, ii_out, nnz_offsets_out, row_offsets_out, cap_out, added,          viol,  ret};
    HIP_TRY(launch_prune_grow(g, p, prune_layout(workspace, batch, N), as_stream(stream_)));
    return 0;
}

int lapwarm_prune_finish_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                const int *x, double *v, const int *ret, double *u, double *cost, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!x || !v || !ret || !u || !cost) return -2;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    HIP_TRY(launch_prune_finish(g, x, v, ret, u, cost, as_stream(stream_)));
    return 0;
}

int lapwarm_project_round_batched(const double *C, int batch, int n, double *u, double *v,
                                  double *gmin, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (int rc = check_workspace(workspace_bytes, lapwarm_sweep_workspace_bytes(batch, n))) return rc;
    hipStream_t stream = as_stream(stream_);
    const SweepWs w = sweep_layout(workspace, batch, n);
    HIP_TRY(launch_cap_rows(C, n, batch, u, v, stream));
    HIP_TRY(launch_cap_cols(C, n, batch, u, v, w.partial, stream));
    HIP_TRY(launch_reduced_min(C, n, batch, u, v, w.rowpart, gmin, stream));
    return 0;
}

int lapwarm_reduce_costs_batched(const double *C, int batch, int n, const double *u, const double *v,
                                 int shift_nonneg, double *out, double *gmin, void *workspace,
                                 size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (int rc = check_workspace(workspace_bytes, lapwarm_sweep_workspace_bytes(batch, n))) return rc;
    hipStream_t stream = as_stream(stream_);
    HIP_TRY(launch_reduced_min(C, n, batch, u, v, sweep_layout(workspace, batch, n).rowpart, gmin, stream));
    HIP_TRY(launch_reduce_costs(C, n, batch, u, v, gmin, shift_nonneg, out, stream));
    return 0;
}

// ---- dual utilities of a ragged batch (ragged_duals.hpp, ragged_batch.hip) ----
static RaggedDualsWs ragged_duals_layout(void *workspace, int batch, int N)
{
    Carver c{reinterpret_cast<unsigned char *>(workspace), 0};
    RaggedDualsWs w;
    w.part = c.take<double>((size_t)batch * N);
    w.done = c.take<int>(batch);
    w.running = c.take<int>(1);
    w.bytes = c.off;
    return w;
}

size_t lapwarm_ragged_duals_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return ragged_duals_layout(nullptr, batch, N).bytes;
}

static int check_ragged_duals_ws(const void *workspace, size_t workspace_bytes, int batch, int N)
{
    if (!workspace) return -2;
    return check_workspace(workspace_bytes, lapwarm_ragged_duals_workspace_bytes(batch, N));
}

int lapwarm_rowmin_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                          const double *v, double *out, int *ret, void *workspace, size_t workspace_bytes,
                          void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!out) return -2;
    if (int rc = check_ragged_duals_ws(workspace, workspace_bytes, batch, N)) return rc;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    HIP_TRY(launch_rowmin_ragged(g, v, out, ret, as_stream(stream_)));
    return 0;
}

// The rounds are launched in chunks (1, then 2, 4, ... 32 at a time) up to max(1, max_rounds), with one host
// synchronisation after each chunk but the last to learn whether any instance still runs: almost every call on
// finite costs ends with the first.  Not graph-capturable.
int lapwarm_project_feasible_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch,
                                    int N, double *u, double *v, int max_rounds, double tol, double *gmin,
                                    int *rounds, int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!u || !v || !gmin || !rounds || !ret) return -2;
    if (int rc = check_ragged_duals_ws(workspace, workspace_bytes, batch, N)) return rc;
    hipStream_t stream = as_stream(stream_);
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    const RaggedDualsWs w = ragged_duals_layout(workspace, batch, N);
    HIP_TRY(launch_project_init_ragged(g, w, u, v, gmin, rounds, ret, stream));
    const int total = (max_rounds < 1) ? 1 : max_rounds;  // max(1, int(max_rounds)), advanced_dual.py:28
    int r = 0, chunk = 1;
    for (;;) {
        const int k = (chunk < total - r) ? chunk : total - r;
        for (int t = 0; t < k; ++t, ++r) HIP_TRY(launch_project_round_ragged(g, w, u, v, tol, gmin, rounds, stream));
        if (r >= total) break;
        int host_running = 0;
        HIP_TRY(hipMemcpyAsync(&host_running, w.running, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (host_running == 0) break;
        if (chunk < 32) chunk *= 2;
    }
    return 0;
}

int lapwarm_reduce_costs_ragged(const double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                const double *u, const double *v, int shift_nonneg, double *out, double *gmin,
                                int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!u || !v || !gmin) return -2;
    if (int rc = check_ragged_duals_ws(workspace, workspace_bytes, batch, N)) return rc;
    const RaggedBatch g{C, offsets, sizes, ld, batch, N};
    const RaggedDualsWs w = ragged_duals_layout(workspace, batch, N);
    HIP_TRY(launch_reduce_costs_ragged(g, w, u, v, shift_nonneg, out, gmin, ret, as_stream(stream_)));
    return 0;
}

// ---- synthetic cost families drawn into a ragged batch (cost_families.hpp) ----
static CostFamiliesWs cost_families_layout(void *workspace, int batch, int N)
{
    Carver c{reinterpret_cast<unsigned char *>(workspace), 0};
    CostFamiliesWs w;
    w.fa = c.take<double>((size_t)batch * N * kMaxRank);
    w.fb = c.take<double>((size_t)batch * N * kMaxRank);
    w.part = c.take<double>((size_t)batch * cost_tiles(N));
    w.colany = c.take<unsigned char>((size_t)batch * N);
    w.bytes = c.off;
    return w;
}

size_t lapwarm_cost_families_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N)) return 0;
    return cost_families_layout(nullptr, batch, N).bytes;
}

int lapwarm_generate_costs_ragged(double *C, const long long *offsets, const int *sizes, int ld, int batch, int N,
                                  const int *family, const unsigned long long *seeds, const double *params, int *ret,
                                  void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!family || !seeds || !params || !ret || !workspace) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_cost_families_workspace_bytes(batch, N))) return rc;
    const CostFamiliesArgs a{C,      offsets, sizes, ld,  batch, N,
                             family, seeds,   params, ret, cost_families_layout(workspace, batch, N)};
    HIP_TRY(launch_generate_costs_ragged(a, as_stream(stream_)));
    return 0;
}

int lapwarm_cost_family_draws(unsigned long long seed, unsigned int stream_id, int kind, unsigned long long first,
                              unsigned long long count, unsigned int m, void *out, void *stream_)
{
    if (kind < 0 || kind > 2 || (kind == 2 && (m < 1 || m > 0x7fffffffu))) return -2;
    if (count == 0) return 0;
    if (!out || count >= (1ull << 39)) return -2;  // the grid's x dimension: 2^31 blocks of 256
    HIP_TRY(launch_cost_family_draws(seed, stream_id, kind, first, count, (int)m, out, as_stream(stream_)));
    return 0;
}

size_t lapwarm_oracle_duals_workspace_bytes(int batch, int n)
{
    if (batch <= 0 || n <= 0) return 0;
    OracleParams p;
    return oracle_layout(nullptr, batch, n, &p).bytes;
}

// Init, the sweeps and the finish of a uniform or a ragged call.  Sweeps are launched in chunks (4, 8, 16, then
// 32 at a time) up to max_s, with one host synchronisation per chunk to learn whether any instance still needs
// sweeps: not graph-capturable.  The one place that knows the schedule: a ragged instance is bit-equal to the
// uniform call because both are checked at the same sweep numbers.
static int oracle_run(const OracleParams &p, const OracleWs &w, int max_s, double tol, double *u, double *v, int *ret,
                      int *sweeps, hipStream_t stream)
{
    HIP_TRY(launch_oracle_init(p, stream));
    int s = 0, chunk = 4;
    for (;;) {
        const int k = (chunk < max_s - s) ? chunk : max_s - s;
        for (int t = 0; t < k; ++t, ++s) HIP_TRY(launch_oracle_sweep(p, s, stream));
        const int last = s >= max_s;
        HIP_TRY(hipMemsetAsync(w.running, 0, sizeof(int), stream));
        HIP_TRY(launch_oracle_check(p, s, last, w.running, stream));
        if (last) break;
        int host_running = 0;
        HIP_TRY(hipMemcpyAsync(&host_running, w.running, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (host_running == 0) break;
        if (chunk < 32) chunk *= 2;
    }
    HIP_TRY(launch_oracle_finish(p, tol, u, v, w.rowpart, w.gmin, ret, sweeps, stream));
    return 0;
}

static int oracle_duals_impl(const double *C, int batch, int n, const int *rows, const int *cols, double *u,
                             double *v, int *ret, int *sweeps, void *workspace, size_t workspace_bytes,
                             double tol, hipStream_t stream)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (int rc = check_workspace(workspace_bytes, lapwarm_oracle_duals_workspace_bytes(batch, n))) return rc;
    OracleParams p;
    p.C = C;
    p.n = n;
    p.batch = batch;
    p.chunks = oracle_chunks(n, batch);
    p.pair = (n % 2) == 0 && (reinterpret_cast<uintptr_t>(C) % 16) == 0;
    p.rows = rows;
    p.cols = cols;
    const OracleWs w = oracle_layout(workspace, batch, n, &p);
    // settled within n - 1 sweeps <=> at most n - 2 updating sweeps
    return oracle_run(p, w, n - 1, tol, u, v, ret, sweeps, stream);
}

int lapwarm_oracle_duals_batched(const double *C, int batch, int n, const int *rows, const int *cols, double *u,
                                 double *v, int *ret, int *sweeps, void *workspace, size_t workspace_bytes,
                                 void *stream_)
{
    return oracle_duals_impl(C, batch, n, rows, cols, u, v, ret, sweeps, workspace, workspace_bytes, 1e-12,
                             as_stream(stream_));
}

size_t lapwarm_oracle_duals_ragged_workspace_bytes(int batch, int N)
{
    if (check_ragged_dims(batch, N) || N > kOracleMaxN) return 0;
    OracleParams p;
    return oracle_layout(nullptr, batch, N, &p).bytes;  // the uniform slots with the padded stride N
}

// One init and one chain of sweep chunks for all instances: the chunk schedule of oracle_run is shared and runs to
// the largest budget, max_b (n_b - 1), taken from the host sizes; the kernels keep every instance to its own
// budget.  As many host synchronisations as one uniform call of the largest size: not graph-capturable.
int lapwarm_oracle_duals_ragged(const double *C, const long long *offsets, const int *sizes, const int *host_sizes,
                                int ld, int batch, int N, const int *rows, const int *cols, double *u, double *v,
                                int *ret, int *sweeps, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_ragged(C, offsets, sizes, ld, batch, N)) return rc;
    if (!host_sizes || !rows || !cols || !u || !v || !ret || !workspace) return -2;
    OracleParams p;
    p.C = C;
    p.n = N;
    p.batch = batch;
    p.chunks = oracle_chunks(N, batch);
    p.pair = 0;  // chosen per instance on the device
    p.offsets = offsets;
    p.sizes = sizes;
    p.ld = ld;
    p.rows = rows;
    p.cols = cols;
    const OracleWs w = oracle_layout(workspace, batch, N, &p);
    if (int rc = check_workspace(workspace_bytes, w.bytes)) return rc;
    // (not host_sizes_ok: this entry skips a host size the device would treat as empty, which asks for no
    // sweeps, where the solves reject the batch)
    int max_s = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = host_sizes[b];
        if (n >= 1 && n <= N && (ld == 0 || n <= ld) && n - 1 > max_s) max_s = n - 1;
    }
    hipStream_t stream = as_stream(stream_);
    return oracle_run(p, w, max_s, 1e-12, u, v, ret, sweeps, stream);
}

size_t lapwarm_train_loss_workspace_bytes(int batch, int n)
{
    if (check_ragged_dims(batch, n)) return 0;  // (the batch is the y dimension of its grids too)
    TrainLossParams p{};
    p.n = n;
    p.batch = batch;
    train_loss_plan(&p);
    return train_loss_layout(nullptr, &p);
}

int lapwarm_train_loss_forward(const float *C, int batch, int n, const int *sizes, const float *u_pred,
                               const float *u_target, float *v_proj, int *argmin_row, int *assign, float *terms,
                               int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (batch > kMaxGridY) return -2;  // the batch is one dimension of every grid
    if (int rc = check_workspace(workspace_bytes, lapwarm_train_loss_workspace_bytes(batch, n))) return rc;
    TrainLossParams p{};
    p.C = C;
    p.n = n;
    p.batch = batch;
    p.sizes = sizes;
    p.u = u_pred;
    p.ut = u_target;
    p.v = v_proj;
    p.arow = argmin_row;
    p.assign = assign;
    p.terms = terms;
    p.ret = ret;
    train_loss_plan(&p);
    train_loss_layout(workspace, &p);
    HIP_TRY(launch_train_loss_forward(p, as_stream(stream_)));
    return 0;
}

int lapwarm_train_loss_backward(int batch, int n, const int *sizes, const float *u_pred, const float *u_target,
                                const float *weights, float grad_scale, float *grad_u, const void *workspace,
                                size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (batch > kMaxGridY) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_train_loss_workspace_bytes(batch, n))) return rc;
    TrainLossParams p{};
    p.n = n;
    p.batch = batch;
    p.sizes = sizes;
    p.u = u_pred;
    p.ut = u_target;
    train_loss_plan(&p);
    train_loss_layout(const_cast<void *>(workspace), &p);  // the kernel only reads it
    HIP_TRY(launch_train_loss_backward(p, weights, grad_scale, grad_u, as_stream(stream_)));
    return 0;
}

size_t lapwarm_dual_loss_workspace_bytes(int batch, int n)
{
    if (check_ragged_dims(batch, n)) return 0;
    TrainLossParams p{};
    p.n = n;
    p.batch = batch;
    train_loss_plan(&p);
    return dual_loss_layout(nullptr, &p);
}

int lapwarm_dual_loss_forward(const float *C, int batch, int n, const int *sizes, const float *u_pred,
                              const float *v_hint, float *v_proj, int *argmin_row, int *assign, float *terms,
                              int *ret, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (batch > kMaxGridY) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_dual_loss_workspace_bytes(batch, n))) return rc;
    TrainLossParams p{};
    p.C = C;
    p.n = n;
    p.batch = batch;
    p.sizes = sizes;
    p.u = u_pred;
    p.vh = v_hint;
    p.v = v_proj;
    p.arow = argmin_row;
    p.assign = assign;
    p.terms = terms;
    p.ret = ret;
    train_loss_plan(&p);
    dual_loss_layout(workspace, &p);
    HIP_TRY(launch_train_loss_forward(p, as_stream(stream_)));
    return 0;
}

int lapwarm_dual_loss_backward(int batch, int n, const int *sizes, const float *u_pred, const float *v_hint,
                               const float *weights, float grad_scale, float *grad_u, float *grad_v_hint,
                               const void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_dims(batch, n)) return rc;
    if (batch > kMaxGridY) return -2;
    if (int rc = check_workspace(workspace_bytes, lapwarm_dual_loss_workspace_bytes(batch, n))) return rc;
    TrainLossParams p{};
    p.n = n;
    p.batch = batch;
    p.sizes = sizes;
    p.u = u_pred;
    p.vh = v_hint;
    train_loss_plan(&p);
    dual_loss_layout(const_cast<void *>(workspace), &p);  // the kernel only reads it
    HIP_TRY(launch_dual_loss_backward(p, weights, grad_scale, grad_u, grad_v_hint, as_stream(stream_)));
    return 0;
}

// ------------------------------------------------------------------------------------------
// Host-pointer drop-ins
// ------------------------------------------------------------------------------------------
int lapjv_seeded(const double *C, int n_rows, int n_cols, long long *x, long long *y,
                 const double *u_seed, const double *v_seed, double eps)
{
    if (n_rows <= 0 || n_cols <= 0) return -2;  // lapjv_seeded.cpp:25
    if (n_rows != n_cols) return -4;            // lapjv_seeded.cpp:27
    const int n = n_rows;
    if (n > kMaxN) return -5;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_seeded_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, du, dv, dx, dy, dret, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(n), c.take<double>(n), c.take<long long>(n),
                          c.take<long long>(n), c.take<int>(1), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    HIP_TRY(upload(du, u_seed, n));
    HIP_TRY(upload(dv, v_seed, n));
    if (int rc = lapwarm_seeded_batched(dC, 1, n, du, dv, eps, dx, dy, dret, nullptr, ws, ws_bytes, 0, nullptr))
        return rc;
    if (int ret = device_ret(dret)) return ret;
    HIP_TRY(download(x, dx, n));
    HIP_TRY(download(y, dy, n));
    return 0;
}

int lapwarm_lapjv_dense(const double *C, int n, int *x, int *y)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_lapjv_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, dx, dy, dret, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<int>(n), c.take<int>(n), c.take<int>(1),
                          c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    if (int rc = lapwarm_lapjv_batched(dC, 1, n, dx, dy, dret, nullptr, ws, ws_bytes, 0, nullptr)) return rc;
    if (int ret = device_ret(dret)) return ret;
    HIP_TRY(download(x, dx, n));
    HIP_TRY(download(y, dy, n));
    return 0;
}

int lapwarm_lapjv_extended(const double *C, int n_rows, int n_cols, int extend_cost, double cost_limit,
                           int *x, int *y, double *opt)
{
    const int n = lapwarm_lapjv_extended_n(n_rows, n_cols, extend_cost, cost_limit);
    if (n < 0) return n;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_lapjv_extended_workspace_bytes(1, n_rows, n_cols, extend_cost, cost_limit);
    const size_t nc = (size_t)n_rows * n_cols;
    // (only C crosses to the device: the extended matrix is built there)
    const auto [dC, dx, dy, dopt, dret, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nc), c.take<int>(n_rows), c.take<int>(n_cols), c.take<double>(1),
                          c.take<int>(1), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nc));
    if (int rc = lapwarm_lapjv_extended_batched(dC, 1, n_rows, n_cols, extend_cost, cost_limit, dx, dy, dopt, nullptr,
                                                dret, nullptr, ws, ws_bytes, 0, nullptr))
        return rc;
    if (int ret = device_ret(dret)) return ret;
    HIP_TRY(download(x, dx, n_rows));
    HIP_TRY(download(y, dy, n_cols));
    if (opt) HIP_TRY(download(opt, dopt, 1));
    return 0;
}

int lapwarm_warmstart_lapjv(const double *C, int n, const double *u, const double *v, int shift_nonneg,
                            int *x, int *y)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_sweep = lapwarm_sweep_workspace_bytes(1, n);
    const size_t ws_solve = lapwarm_lapjv_workspace_bytes(1, n), nn = (size_t)n * n;
    // (dR, the reduced matrix, never leaves the device)
    const auto [dC, dR, du, dv, dg, dx, dy, dret, wsA, wsB] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(nn), c.take<double>(n), c.take<double>(n),
                          c.take<double>(1), c.take<int>(n), c.take<int>(n), c.take<int>(1),
                          c.take<unsigned char>(ws_sweep), c.take<unsigned char>(ws_solve)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    HIP_TRY(upload(du, u, n));
    HIP_TRY(upload(dv, v, n));
    if (int rc = lapwarm_reduce_costs_batched(dC, 1, n, du, dv, shift_nonneg, dR, dg, wsA, ws_sweep, nullptr))
        return rc;
    if (int rc = lapwarm_lapjv_batched(dR, 1, n, dx, dy, dret, nullptr, wsB, ws_solve, 0, nullptr)) return rc;
    if (int ret = device_ret(dret)) return ret;
    HIP_TRY(download(x, dx, n));
    HIP_TRY(download(y, dy, n));
    return 0;
}

static void host_posenc(int n, float *out)
{
    // gnn/features.py:21-31, fp64 then float32
    static const int freqs[4] = {1, 2, 4, 8};
    const double scale = (n - 1 > 1) ? (double)(n - 1) : 1.0;
    for (int i = 0; i < n; ++i) {
        for (int f = 0; f < 4; ++f) {
            const double ang = 2.0 * M_PI * (double)i * (double)freqs[f] / scale;
            out[(size_t)i * 8 + 2 * f] = (float)sin(ang);
            out[(size_t)i * 8 + 2 * f + 1] = (float)cos(ang);
        }
    }
}

int lapwarm_row_features(const double *C, int n, float *feat, float *topk16)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_sweep_workspace_bytes(1, n), rows = (size_t)n;
    const auto [dC, dpos, dfeat, dtop, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(rows * n), c.take<float>(rows * 8), c.take<float>(rows * 21),
                          c.take<float>(rows * 16), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    std::vector<float> pos(rows * 8);
    host_posenc(n, pos.data());
    HIP_TRY(upload(dpos, pos.data(), pos.size()));
    HIP_TRY(upload(dC, C, rows * n));
    if (int rc = lapwarm_row_features_batched(dC, 1, n, dpos, dfeat, dtop, ws, ws_bytes, nullptr)) return rc;
    HIP_TRY(download(feat, dfeat, rows * 21));
    if (topk16) HIP_TRY(download(topk16, dtop, rows * 16));
    return 0;
}

int lapwarm_min_trick(const double *C, int n, const double *u, double *v)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_sweep_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, du, dv, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(n), c.take<double>(n), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    if (u) HIP_TRY(upload(du, u, n));
    if (int rc = lapwarm_colmin_batched(dC, 1, n, u ? du : nullptr, dv, ws, ws_bytes, nullptr)) return rc;
    HIP_TRY(download(v, dv, n));
    return 0;
}

int lapwarm_row_min(const double *C, int n, const double *v, double *out)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t nn = (size_t)n * n;
    const auto [dC, dv, dout] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(n), c.take<double>(n)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    if (v) HIP_TRY(upload(dv, v, n));
    if (int rc = lapwarm_rowmin_batched(dC, 1, n, v ? dv : nullptr, dout, nullptr)) return rc;
    HIP_TRY(download(out, dout, n));
    return 0;
}

int lapwarm_project_feasible(const double *C, int n, double *u, double *v, int max_rounds, double tol)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_sweep_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, du, dv, dg, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(n), c.take<double>(n), c.take<double>(1),
                          c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    HIP_TRY(upload(du, u, n));
    HIP_TRY(upload(dv, v, n));
    const int rounds = (max_rounds < 1) ? 1 : max_rounds;  // max(1, int(max_rounds)), advanced_dual.py:28
    for (int r = 0; r < rounds; ++r) {
        if (int rc = lapwarm_project_round_batched(dC, 1, n, du, dv, dg, ws, ws_bytes, nullptr)) return rc;
        double g = 0.0;
        HIP_TRY(download(&g, dg, 1));
        if (g >= -tol) break;
    }
    HIP_TRY(download(u, du, n));
    HIP_TRY(download(v, dv, n));
    return 0;
}

int lapwarm_reduce_costs(const double *C, int n, const double *u, const double *v, int shift_nonneg,
                         double *out, double *min_out)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_sweep_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, dO, du, dv, dg, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<double>(nn), c.take<double>(n), c.take<double>(n),
                          c.take<double>(1), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    HIP_TRY(upload(du, u, n));
    HIP_TRY(upload(dv, v, n));
    if (int rc = lapwarm_reduce_costs_batched(dC, 1, n, du, dv, shift_nonneg, dO, dg, ws, ws_bytes, nullptr))
        return rc;
    if (out) HIP_TRY(download(out, dO, nn));
    if (min_out) HIP_TRY(download(min_out, dg, 1));
    return 0;
}

int lapwarm_oracle_duals(const double *C, int n, const int *rows, const int *cols, double *u, double *v,
                         double tol)
{
    if (int rc = check_dims(1, n)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t ws_bytes = lapwarm_oracle_duals_workspace_bytes(1, n), nn = (size_t)n * n;
    const auto [dC, dr, dc, du, dv, dret, ws] = g_arena.stage([&](Carver &c) {
        return std::tuple{c.take<double>(nn), c.take<int>(n), c.take<int>(n), c.take<double>(n), c.take<double>(n),
                          c.take<int>(1), c.take<unsigned char>(ws_bytes)};
    });
    if (!dC) return -1;
    HIP_TRY(upload(dC, C, nn));
    HIP_TRY(upload(dr, rows, n));
    HIP_TRY(upload(dc, cols, n));
    if (int rc = oracle_duals_impl(dC, 1, n, dr, dc, du, dv, dret, nullptr, ws, ws_bytes, tol, nullptr)) return rc;
    if (int ret = device_ret(dret)) return ret;
    HIP_TRY(download(u, du, n));
    HIP_TRY(download(v, dv, n));
    return 0;
}

}  // extern "C"
