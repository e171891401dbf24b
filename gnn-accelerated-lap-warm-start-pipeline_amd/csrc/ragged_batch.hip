// ragged_batch.hip -- the dense sweeps that exist only for a batch of cost matrices of different sizes, gfx950:
// column minima, the reduced-cost minimum, and the dual utilities (row minima, feasibility projection, reduced
// costs).  Every kernel is one grid over all instances.
//
// Reference behaviour reproduced (paths relative to the reference project): the column minima of
// gnn/features.py:218 and the min-trick of scripts/gnn_benchmark.py:262; solvers/advanced_dual.py:14-63
// (project_feasible, reduce_costs, check_dual_feasible) and the row minima of solvers/seed_baselines.py:29, per
// instance of a batch laid out as `collate` (gnn/train_one_gnn.py:72-91) pads it or packed back to back
// (ragged_batch.hpp).
//
// A round of project_feasible reads C twice, not three times.  The column pass has cap_j = min_i fl(C_ij - u_i)
// in hand when it writes v_j = min(v_j, cap_j); x -> fl(x - v_j) is monotone, so
//     min_i fl(fl(C_ij - u_i) - v_j) = fl(cap_j - v_j)   and   min((C - u) - v) = min_j fl(cap_j - v_j).
// It holds with NaN (a NaN term makes cap_j, v_j and both sides NaN) and with infinities (a term inf - inf needs
// fl(C_ij - u_i) = v_j = +-inf, and v_j <= cap_j <= fl(C_ij - u_i) then forces cap_j = v_j: NaN on both sides).
#include "device_utils.hpp"
#include "ragged_duals.hpp"

namespace lapwarm {

namespace {

constexpr int kTileCols = 32;   // columns of one workgroup: 256 B of every row it reads
constexpr int kTileSlices = 16; // row slices: slice s reads rows s, s + 16, ...
constexpr int kTileThreads = kTileCols / 2 * kTileSlices;

// The column tile: min_{i < n} (C_b[i][j] - (HAS_U ? u[b][i] : 0)) of column j = j0 + threadIdx.x, returned to the
// threads below kTileCols (the others get nothing of use).  j0 < n, and the whole workgroup calls it.
// The workgroups are narrow column tiles over all rows of one instance and the 16 row slices meet in LDS.  A lane
// owns two columns.  Where the instance's base and row stride are both multiples of 16 bytes they are neighbours
// and come in one 16-byte load; otherwise they lie 16 columns apart and come in two 8-byte loads, each still
// contiguous over 16 lanes.  The choice is per instance, from its offset and size on the device.
template <bool HAS_U>
__device__ __forceinline__ double col_tile_min(const RaggedBatch &g, const double *u, int b, int j0, int n,
                                               double (*red)[kTileCols + 1])
{
    const int tx = threadIdx.x & (kTileCols / 2 - 1), ty = threadIdx.x / (kTileCols / 2);
    const size_t stride = g.ld ? g.ld : n;
    const double *base = g.C + g.offsets[b];
    const bool aligned = (reinterpret_cast<uintptr_t>(base) % 16) == 0 && (stride % 2) == 0;
    const int c0 = aligned ? 2 * tx : tx, c1 = aligned ? 2 * tx + 1 : tx + kTileCols / 2;
    const bool in0 = j0 + c0 < n, in1 = j0 + c1 < n;
    const double *ub = HAS_U ? u + (size_t)b * g.N : nullptr;
    double m0 = pos_inf(), m1 = pos_inf();
    if (aligned && in1) {
        const double *p = base + j0 + c0;
#pragma unroll 4
        for (int i = ty; i < n; i += kTileSlices) {
            const double2 c = *reinterpret_cast<const double2 *>(p + (size_t)i * stride);
            const double ui = HAS_U ? ub[i] : 0.0;
            m0 = nmin(m0, HAS_U ? c.x - ui : c.x);
            m1 = nmin(m1, HAS_U ? c.y - ui : c.y);
        }
    } else if (in0) {
        const double *p = base + j0;
#pragma unroll 4
        for (int i = ty; i < n; i += kTileSlices) {
            const double *r = p + (size_t)i * stride;
            const double x = r[c0];
            const double y = in1 ? r[c1] : pos_inf();
            const double ui = HAS_U ? ub[i] : 0.0;
            m0 = nmin(m0, HAS_U ? x - ui : x);
            if (in1) m1 = nmin(m1, HAS_U ? y - ui : y);
        }
    }
    red[ty][c0] = m0;
    red[ty][c1] = m1;
    __syncthreads();
    double m = pos_inf();
    if (threadIdx.x < kTileCols) {
        m = red[0][threadIdx.x];
#pragma unroll
        for (int s = 1; s < kTileSlices; ++s) m = nmin(m, red[s][threadIdx.x]);
    }
    return m;
}

// out[b][j] = the column minimum on the prefix, 0 up to N.  One kernel, where the uniform batch has two (row
// chunks, then their combination): B * N / 32 workgroups.
template <bool HAS_U>
__global__ void __launch_bounds__(kTileThreads) colmin_ragged_kernel(RaggedBatch g, const double *u, double *out)
{
    __shared__ double red[kTileSlices][kTileCols + 1];
    const int b = blockIdx.y, j0 = blockIdx.x * kTileCols, N = g.N;
    const int n = ragged_size(g, b);
    const bool mine = threadIdx.x < kTileCols && j0 + threadIdx.x < N;
    if (j0 >= n) {  // a tile right of the prefix: workgroup-uniform
        if (mine) out[(size_t)b * N + j0 + threadIdx.x] = 0.0;
        return;
    }
    const double m = col_tile_min<HAS_U>(g, u, b, j0, n, red);
    if (mine) out[(size_t)b * N + j0 + threadIdx.x] = (j0 + threadIdx.x < n) ? m : 0.0;
}

// The column pass of a round: the tile caps its 32 entries of v and leaves cap_j - v_j, the column's share of
// gmin, in part.
__global__ void __launch_bounds__(kTileThreads)
col_cap_ragged_kernel(RaggedBatch g, const double *u, double *v, double *part, const int *done)
{
    __shared__ double red[kTileSlices][kTileCols + 1];
    const int b = blockIdx.y, j0 = blockIdx.x * kTileCols;
    if (done[b]) return;
    const int n = ragged_size(g, b);
    if (j0 >= n) return;  // a tile right of the prefix: workgroup-uniform
    const double cap = col_tile_min<true>(g, u, b, j0, n, red);
    if (threadIdx.x < kTileCols && j0 + threadIdx.x < n) {
        const size_t o = (size_t)b * g.N + j0 + threadIdx.x;
        const double vj = nmin(v[o], cap);
        v[o] = vj;
        part[o] = cap - vj;
    }
}

constexpr int kRowThreads = 256;

enum RowKind {
    kRowMin = 0,      // out[b][i]  = min_j (C - v_j), 0 beyond the prefix; v may be null
    kRowCap = 1,      // u[b][i]    = min(u[b][i], min_j (C - v_j)) unless done[b]
    kRowReduced = 2,  // part[b][i] = min_j ((C - u_i) - v_j)
};

struct RowArgs {
    const double *u;  // kRowReduced
    const double *v;
    double *out;      // out, u or part
    int *ret;         // kRowMin, may be null
    const int *done;  // kRowCap
    int *running;     // kRowCap: reset here, set again by the kernel that ends the round
};

// Workgroup (i, b) owns row i of instance b.  Where the instance's base and row stride are multiples of 16 bytes a
// lane reads two neighbouring columns in one 16-byte load, otherwise one column in an 8-byte load: per instance,
// from its offset and size on the device, as the column tile chooses.
template <int KIND>
__global__ void __launch_bounds__(kRowThreads) row_pass_ragged_kernel(RaggedBatch g, RowArgs a)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.y, i = blockIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
    const size_t o = (size_t)b * g.N + i;
    if constexpr (KIND == kRowCap) {
        if (i == 0 && b == 0 && threadIdx.x == 0) *a.running = 0;
        if (a.done[b]) return;
    }
    if constexpr (KIND == kRowMin) {
        if (i == 0 && threadIdx.x == 0 && a.ret) a.ret[b] = n ? 0 : 2;
        if (i >= n) {
            if (threadIdx.x == 0) a.out[o] = 0.0;
            return;
        }
    }
    if (i >= n) return;
    BlockCtx bc;
    bc.init(&ex);
    const size_t stride = g.ld ? g.ld : n;
    const double *base = g.C + g.offsets[b];
    const double *row = base + (size_t)i * stride;
    const double *vb = a.v ? a.v + (size_t)b * g.N : nullptr;
    const double ui = (KIND == kRowReduced) ? a.u[o] : 0.0;
    auto term = [&](double c, int j) {
        if constexpr (KIND == kRowReduced) return (c - ui) - vb[j];
        return vb ? c - vb[j] : c;
    };
    const bool aligned = (reinterpret_cast<uintptr_t>(base) % 16) == 0 && (stride % 2) == 0;
    double m = pos_inf();
    if (aligned) {
        const int n2 = n & ~1;
#pragma unroll 2
        for (int j = 2 * bc.tid; j < n2; j += 2 * kRowThreads) {
            const double2 c = *reinterpret_cast<const double2 *>(row + j);
            m = nmin(m, term(c.x, j));
            m = nmin(m, term(c.y, j + 1));
        }
        if ((n & 1) && bc.tid == 0) m = nmin(m, term(row[n - 1], n - 1));
    } else {
#pragma unroll 2
        for (int j = bc.tid; j < n; j += kRowThreads) m = nmin(m, term(row[j], j));
    }
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) a.out[o] = (KIND == kRowCap) ? nmin(a.out[o], m) : m;
}

// gmin[b] = min of the prefix of part[b]: one workgroup per instance.  PROJECT: the end of a round, which counts
// it and decides whether the instance stops (`gmin >= -tol`, which NaN fails).  Otherwise the minimum behind
// reduce_costs, with 0 and ret 2 for an instance treated as empty.
template <bool PROJECT>
__global__ void __launch_bounds__(kRowThreads)
gmin_ragged_kernel(RaggedBatch g, const double *part, double *gmin, double tol, int *rounds, int *done, int *running,
                   int *ret)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.x;
    const int n = ragged_size(g, b);
    if constexpr (PROJECT) {
        if (done[b]) return;
    } else if (n == 0) {
        if (threadIdx.x == 0) {
            gmin[b] = 0.0;
            if (ret) ret[b] = 2;
        }
        return;
    }
    BlockCtx bc;
    bc.init(&ex);
    double m = pos_inf();
    for (int j = bc.tid; j < n; j += kRowThreads) m = nmin(m, part[(size_t)b * g.N + j]);
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) {
        gmin[b] = m;
        if constexpr (PROJECT) {
            rounds[b] += 1;
            if (m >= -tol)
                done[b] = 1;
            else
                *running = 1;  // (every writer writes 1)
        } else if (ret) {
            ret[b] = 0;
        }
    }
}

__global__ void __launch_bounds__(kRowThreads)
project_init_ragged_kernel(RaggedBatch g, double *u, double *v, double *gmin, int *rounds, int *ret, int *done)
{
    const int b = blockIdx.y, j = blockIdx.x * kRowThreads + threadIdx.x;
    const int n = ragged_size(g, b);
    if (j >= n && j < g.N) {
        u[(size_t)b * g.N + j] = 0.0;
        v[(size_t)b * g.N + j] = 0.0;
    }
    if (j == 0) {
        done[b] = n == 0;
        rounds[b] = 0;
        ret[b] = n ? 0 : 2;
        gmin[b] = 0.0;
    }
}

// out = (C - u_i) - v_j on the prefix, minus min(out) when that is negative (advanced_dual.py:47-53)
__global__ void __launch_bounds__(kRowThreads)
reduce_costs_ragged_kernel(RaggedBatch g, const double *u, const double *v, const double *gmin, int shift_nonneg,
                           double *out)
{
    const int b = blockIdx.y, i = blockIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
    if (i >= n) return;
    const size_t off = (size_t)g.offsets[b] + (size_t)i * (g.ld ? g.ld : n);
    const double ui = u[(size_t)b * g.N + i];
    const double *vb = v + (size_t)b * g.N;
    const double gm = gmin[b];
    const bool shift = shift_nonneg && (gm < 0);
    for (int j = threadIdx.x; j < n; j += kRowThreads) {
        double r = (g.C[off + j] - ui) - vb[j];
        if (shift) r = r - gm;
        out[off + j] = r;
    }
}

// The row pass of the reduced costs, then their minimum per instance: dims checked by the caller
void reduced_min_ragged(const RaggedBatch &g, const double *u, const double *v, double *rowpart, double *gmin,
                        int *ret, hipStream_t stream)
{
    const RowArgs a{u, v, rowpart, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(row_pass_ragged_kernel<kRowReduced>, dim3(g.N, g.batch), dim3(kRowThreads), 0, stream, g, a);
    hipLaunchKernelGGL(gmin_ragged_kernel<false>, dim3(g.batch), dim3(kRowThreads), 0, stream, g, rowpart, gmin, 0.0,
                       (int *)nullptr, (int *)nullptr, (int *)nullptr, ret);
}

}  // namespace

hipError_t launch_colmin_ragged(const RaggedBatch &g, const double *u, double *out, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    const dim3 grid((g.N + kTileCols - 1) / kTileCols, g.batch), block(kTileThreads);
    if (u)
        hipLaunchKernelGGL(colmin_ragged_kernel<true>, grid, block, 0, stream, g, u, out);
    else
        hipLaunchKernelGGL(colmin_ragged_kernel<false>, grid, block, 0, stream, g, u, out);
    return hipGetLastError();
}

hipError_t launch_reduced_min_ragged(const RaggedBatch &g, const double *u, const double *v, double *rowpart,
                                     double *gmin, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    reduced_min_ragged(g, u, v, rowpart, gmin, nullptr, stream);
    return hipGetLastError();
}

hipError_t launch_rowmin_ragged(const RaggedBatch &g, const double *v, double *out, int *ret, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    const RowArgs a{nullptr, v, out, ret, nullptr, nullptr};
    hipLaunchKernelGGL(row_pass_ragged_kernel<kRowMin>, dim3(g.N, g.batch), dim3(kRowThreads), 0, stream, g, a);
    return hipGetLastError();
}

hipError_t launch_project_init_ragged(const RaggedBatch &g, const RaggedDualsWs &w, double *u, double *v, double *gmin,
                                      int *rounds, int *ret, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(project_init_ragged_kernel, dim3((g.N + kRowThreads - 1) / kRowThreads, g.batch),
                       dim3(kRowThreads), 0, stream, g, u, v, gmin, rounds, ret, w.done);
    return hipGetLastError();
}

hipError_t launch_project_round_ragged(const RaggedBatch &g, const RaggedDualsWs &w, double *u, double *v, double tol,
                                       double *gmin, int *rounds, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    const RowArgs a{nullptr, v, u, nullptr, w.done, w.running};
    hipLaunchKernelGGL(row_pass_ragged_kernel<kRowCap>, dim3(g.N, g.batch), dim3(kRowThreads), 0, stream, g, a);
    hipLaunchKernelGGL(col_cap_ragged_kernel, dim3((g.N + kTileCols - 1) / kTileCols, g.batch), dim3(kTileThreads), 0,
                       stream, g, u, v, w.part, w.done);
    hipLaunchKernelGGL(gmin_ragged_kernel<true>, dim3(g.batch), dim3(kRowThreads), 0, stream, g, w.part, gmin, tol,
                       rounds, w.done, w.running, (int *)nullptr);
    return hipGetLastError();
}

hipError_t launch_reduce_costs_ragged(const RaggedBatch &g, const RaggedDualsWs &w, const double *u, const double *v,
                                      int shift_nonneg, double *out, double *gmin, int *ret, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    reduced_min_ragged(g, u, v, w.part, gmin, ret, stream);
    if (out)
        hipLaunchKernelGGL(reduce_costs_ragged_kernel, dim3(g.N, g.batch), dim3(kRowThreads), 0, stream, g, u, v, gmin,
                           shift_nonneg, out);
    return hipGetLastError();
}

}  // namespace lapwarm
