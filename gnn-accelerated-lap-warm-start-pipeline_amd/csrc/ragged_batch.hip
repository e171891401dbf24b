// ragged_batch.hip -- column minima and the reduced-cost minimum of a batch of cost matrices of different sizes,
// gfx950.
//
// Reference behaviour reproduced (paths relative to /root/reference): the column minima of
// gnn/features.py:218 and the min-trick of scripts/gnn_benchmark.py:262, per instance of a batch laid out
// as `collate` (gnn/train_one_gnn.py:72-91) pads it or packed back to back.
#include "device_utils.hpp"
#include "ragged_batch.hpp"

namespace lapwarm {

namespace {

constexpr int kTileCols = 32;   // columns of one workgroup: 256 B of every row it reads
constexpr int kTileSlices = 16; // row slices: slice s reads rows s, s + 16, ...
constexpr int kColminThreads = kTileCols / 2 * kTileSlices;

// One kernel, where the uniform batch has two (row chunks, then their combination): the workgroups are
// narrow column tiles over all rows of one instance, B * N / 32 of them, and the 16 row slices meet in LDS.
// A lane owns two columns.  Where the instance's base and row stride are both multiples of 16 bytes they are
// neighbours and come in one 16-byte load; otherwise they lie 16 columns apart and come in two 8-byte loads,
// each still contiguous over 16 lanes.  The choice is per instance, from its offset and size on the device.
template <bool HAS_U>
__global__ void __launch_bounds__(kColminThreads) colmin_ragged_kernel(RaggedBatch g, const double *u, double *out)
{
    __shared__ double red[kTileSlices][kTileCols + 1];
    const int b = blockIdx.y, j0 = blockIdx.x * kTileCols, N = g.N;
    const int n = ragged_size(g, b);
    const int tx = threadIdx.x & (kTileCols / 2 - 1), ty = threadIdx.x / (kTileCols / 2);
    if (j0 >= n) {  // a tile right of the prefix: workgroup-uniform
        if (threadIdx.x < kTileCols && j0 + threadIdx.x < N) out[(size_t)b * N + j0 + threadIdx.x] = 0.0;
        return;
    }
    const size_t stride = g.ld ? g.ld : n;
    const double *base = g.C + g.offsets[b];
    const bool aligned = (reinterpret_cast<uintptr_t>(base) % 16) == 0 && (stride % 2) == 0;
    const int c0 = aligned ? 2 * tx : tx, c1 = aligned ? 2 * tx + 1 : tx + kTileCols / 2;
    const bool in0 = j0 + c0 < n, in1 = j0 + c1 < n;
    const double *ub = HAS_U ? u + (size_t)b * N : nullptr;
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
    if (threadIdx.x < kTileCols && j0 + threadIdx.x < N) {
        const int c = threadIdx.x;
        double m = red[0][c];
#pragma unroll
        for (int s = 1; s < kTileSlices; ++s) m = nmin(m, red[s][c]);
        out[(size_t)b * N + j0 + c] = (j0 + c < n) ? m : 0.0;
    }
}

constexpr int kRowThreads = 256;

// rowpart[b][i] = min_{j < n_b} ((C_b[i][j] - u_i) - v_j): workgroup (i, b), gone at once beyond the prefix.
__global__ void __launch_bounds__(kRowThreads)
reduced_rowmin_ragged_kernel(RaggedBatch g, const double *u, const double *v, double *rowpart)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.y, i = blockIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
    if (i >= n) return;
    BlockCtx bc;
    bc.init(&ex);
    const double *row = g.C + g.offsets[b] + (size_t)i * (g.ld ? g.ld : n);
    const double *vb = v + (size_t)b * g.N;
    const double ui = u[(size_t)b * g.N + i];
    double m = pos_inf();
    for (int j = bc.tid; j < n; j += kRowThreads) m = nmin(m, (row[j] - ui) - vb[j]);
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) rowpart[(size_t)b * g.N + i] = m;
}

__global__ void __launch_bounds__(kRowThreads) vecmin_ragged_kernel(RaggedBatch g, const double *in, double *out)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.x;
    const int n = ragged_size(g, b);
    BlockCtx bc;
    bc.init(&ex);
    double m = pos_inf();
    for (int j = bc.tid; j < n; j += kRowThreads) m = nmin(m, in[(size_t)b * g.N + j]);
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) out[b] = m;
}

}  // namespace

hipError_t launch_reduced_min_ragged(const RaggedBatch &g, const double *u, const double *v, double *rowpart,
                                     double *gmin, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reduced_rowmin_ragged_kernel, dim3(g.N, g.batch), dim3(kRowThreads), 0, stream, g, u, v,
                       rowpart);
    hipLaunchKernelGGL(vecmin_ragged_kernel, dim3(g.batch), dim3(kRowThreads), 0, stream, g, rowpart, gmin);
    return hipGetLastError();
}

hipError_t launch_colmin_ragged(const RaggedBatch &g, const double *u, double *out, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    const dim3 grid((g.N + kTileCols - 1) / kTileCols, g.batch), block(kColminThreads);
    if (u)
        hipLaunchKernelGGL(colmin_ragged_kernel<true>, grid, block, 0, stream, g, u, out);
    else
        hipLaunchKernelGGL(colmin_ragged_kernel<false>, grid, block, 0, stream, g, u, out);
    return hipGetLastError();
}

}  // namespace lapwarm
