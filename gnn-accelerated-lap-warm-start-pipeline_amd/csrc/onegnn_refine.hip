// onegnn_refine.hip -- aggregation half of OneGNN's top-k refinement (gnn/one_gnn.py:139-155).
//
// For every row: 16 reduced costs -> softmax weights -> sum_k w_k * GELU(w1*val_k + b1) as an
// H-vector.  The reference materialises a (B, n, 16, H) edge embedding and pushes it through an
// H x H GEMM; because that second layer is linear, it commutes with the weighted sum, so this
// kernel emits the (B, n, H) aggregate and the GEMM runs once per row (16x fewer flops, no
// 16x intermediate in HBM).  float32 throughout, exact-erf GELU as torch's default.
#include "device_utils.hpp"
#include "onegnn_refine.hpp"

namespace lapwarm {
namespace {

constexpr int kRefineThreads = 256;
constexpr int kRowsPerBlock = 16;
constexpr int kK = 16;

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__global__ void __launch_bounds__(kRefineThreads)
refine_aggregate_kernel(const float *topk, const float *u_pre, const float *w1, const float *b1,
                        float *out, float *wsum, int rows, int H)
{
    __shared__ float s_val[kRowsPerBlock][kK];
    __shared__ float s_w[kRowsPerBlock][kK];
    const int row0 = blockIdx.x * kRowsPerBlock;
    const int tid = threadIdx.x;
    // phase 1: one 16-lane group per row computes the softmax weights
    {
        const int r = tid >> 4, k = tid & 15;
        const int row = row0 + r;
        float val = __int_as_float(0x7f800000);
        if (row < rows) val = topk[(size_t)row * kK + k] - u_pre[row];
        const bool ok = isfinite(val);
        float mn = ok ? val : __int_as_float(0x7f800000);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, 16));
        float e = ok ? expf(-(val - mn)) : 0.0f;
        float sum = e;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 16);
        const float w = (ok && sum > 0.0f) ? e / sum : 0.0f;
        s_val[r][k] = ok ? val : 0.0f;
        s_w[r][k] = w;
    }
    __syncthreads();
    if (wsum && tid < kRowsPerBlock && row0 + tid < rows) {
        float tot = 0.0f;
#pragma unroll
        for (int k = 0; k < kK; ++k) tot += s_w[tid][k];
        wsum[row0 + tid] = tot;
    }
    // phase 2: every thread walks (row, h) pairs of this block
    const int total = kRowsPerBlock * H;
    for (int idx = tid; idx < total; idx += kRefineThreads) {
        const int r = idx / H, h = idx - r * H;
        const int row = row0 + r;
        if (row >= rows) break;
        const float a = w1[h], c = b1[h];
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < kK; ++k) acc += s_w[r][k] * gelu_erf(a * s_val[r][k] + c);
        out[(size_t)row * H + h] = acc;
    }
}

// ------------------------------------------------------------------------------------------
// Backward of the aggregation.  With G = dL/dout (rows, H) and s = dL/dwsum (rows,):
//   Q_k = sum_h G_h GELU(x_kh) + s      D_k = sum_h G_h w1_h GELU'(x_kh)      GELU'(x) = Phi(x) + x phi(x)
//   dval_k = w_k D_k - w_k (Q_k - sum_m w_m Q_m)   (0 where val_k is not finite),   grad_u = -sum_k dval_k
//   grad_w1[h] = sum_r sum_k G_rh w_rk GELU'(x_rkh) val_rk       grad_b1[h] = sum_r sum_k G_rh w_rk GELU'(x_rkh)
// val, w and both GELU factors are recomputed from the 64 B of a row; nothing of size rows x 16 x H exists.
//
// A workgroup of T = 64..256 threads walks tiles of 16 rows.  Per tile: the forward's phase 1 (a 16-lane
// group per row), then thread t owns the columns h = t, t + T, ... and loops over the live rows of the tile
// with val_k, w_k as LDS broadcasts.  It keeps Q_k and D_k of the row in 32 registers; a butterfly that
// halves the number of values at every step leaves the wave's sum of value i in lane 2 i, which
// adds it to its own LDS slot.  After a barrier the 16-lane group of a row adds the waves' slots in wave
// order and finishes grad_u.  The sums over k and the 16 rows of a tile for grad_w1 / grad_b1 stay with the
// thread (float32 over k, fp64 over rows) and are added to the workgroup's own slab of the workspace, fp64,
// [block][2][H]; refine_backward_sum_kernel adds the slabs in a fixed order and rounds once.  No atomics:
// every sum has one owner and one order, so two runs give the same bits.
// ------------------------------------------------------------------------------------------
constexpr int kBwdMaxBlocks = 2048;
constexpr int kBwdMaxThreads = 256;
constexpr int kSumSlices = 16;  // refine_backward_sum_kernel: 64 columns x 16 slices of slabs

__global__ void __launch_bounds__(kBwdMaxThreads)
refine_backward_kernel(const float *topk, const float *u_pre, const float *w1, const float *b1, const float *G,
                       const float *gws, float *grad_u, double *slabs, int rows, int H, int tiles)
{
    __shared__ float s_val[kRowsPerBlock][kK];
    __shared__ float s_w[kRowsPerBlock][kK];
    __shared__ int s_ok[kRowsPerBlock][kK];
    __shared__ int s_live[kRowsPerBlock];
    __shared__ float s_qd[kBwdMaxThreads / kWave][kRowsPerBlock][2 * kK];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kWave - 1), wave = tid >> 6, nwaves = T >> 6;
    double *slab = slabs + (size_t)blockIdx.x * 2 * H;
    bool first_tile = true;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x, first_tile = false) {
        const int row0 = tile * kRowsPerBlock;
        __syncthreads();  // the previous tile's phase 3 has read s_w, s_ok and s_qd
        for (int p = tid; p < kRowsPerBlock * kK; p += T) {
            const int r = p >> 4, k = p & 15;
            const int row = row0 + r;
            float val = __int_as_float(0x7f800000);
            if (row < rows) val = topk[(size_t)row * kK + k] - u_pre[row];
            const bool ok = isfinite(val);
            float mn = ok ? val : __int_as_float(0x7f800000);
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, 16));
            float e = ok ? expf(-(val - mn)) : 0.0f;
            float sum = e;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 16);
            s_val[r][k] = ok ? val : 0.0f;
            s_w[r][k] = (ok && sum > 0.0f) ? e / sum : 0.0f;
            s_ok[r][k] = ok;
            if (k == 0) s_live[r] = sum > 0.0f;
        }
        __syncthreads();
        bool first_chunk = true;
        for (int h0 = 0; h0 < H; h0 += T, first_chunk = false) {
            const int h = h0 + tid;
            const bool in = h < H;
            const float a = in ? w1[h] : 0.0f, c = in ? b1[h] : 0.0f;
            double acc_w = 0.0, acc_b = 0.0;
            for (int r = 0; r < kRowsPerBlock; ++r) {
                if (!s_live[r]) continue;  // the same for every thread: a row without a finite value adds nothing
                const float g = in ? G[(size_t)(row0 + r) * H + h] : 0.0f;
                const float ga = g * a;
                float v[2 * kK];
                float sw = 0.0f, sb = 0.0f;
#pragma unroll
                for (int k = 0; k < kK; ++k) {
                    const float val = s_val[r][k], w = s_w[r][k];
                    const float x = a * val + c;
                    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
                    const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
                    const float dg = cdf + x * pdf;
                    v[k] = g * (x * cdf);
                    v[kK + k] = ga * dg;
                    const float t = (g * w) * dg;
                    sb += t;
                    sw += t * val;
                }
                acc_w += (double)sw;
                acc_b += (double)sb;
                // 32 values x 64 lanes -> the wave's 32 sums, one per even lane
#pragma unroll
                for (int s = kK, m = 32; s >= 1; s >>= 1, m >>= 1) {
                    const bool upper = (lane & m) != 0;
#pragma unroll
                    for (int i = 0; i < s; ++i) {
                        const float send = upper ? v[i] : v[i + s];
                        const float keep = upper ? v[i + s] : v[i];
                        v[i] = keep + __shfl_xor(send, m, kWave);
                    }
                }
                const float tot = v[0] + __shfl_xor(v[0], 1, kWave);
                if ((lane & 1) == 0) {
                    float *slot = &s_qd[wave][r][lane >> 1];
                    *slot = first_chunk ? tot : *slot + tot;
                }
            }
            if (in) {
                slab[h] = first_tile ? acc_w : slab[h] + acc_w;
                slab[H + h] = first_tile ? acc_b : slab[H + h] + acc_b;
            }
        }
        __syncthreads();
        for (int p = tid; p < kRowsPerBlock * kK; p += T) {
            const int r = p >> 4, k = p & 15;
            const int row = row0 + r;
            const bool live = s_live[r] != 0;
            float q = 0.0f, d = 0.0f;
            if (live) {
                for (int w = 0; w < nwaves; ++w) {
                    q += s_qd[w][r][k];
                    d += s_qd[w][r][kK + k];
                }
                q += gws ? gws[row] : 0.0f;
            }
            const float wk = s_w[r][k];
            float mean = wk * q;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) mean += __shfl_xor(mean, m, 16);
            float dval = (live && s_ok[r][k]) ? wk * d - wk * (q - mean) : 0.0f;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) dval += __shfl_xor(dval, m, 16);
            if (k == 0 && row < rows) grad_u[row] = 0.0f - dval;
        }
    }
}

// grid: one workgroup per 64 columns; thread (slice, lane) adds the slabs slice, slice + 16, ... of its column
// in ascending order, then lanes of slice 0 add the 16 slice sums in slice order.  All fp64, rounded once.
__global__ void __launch_bounds__(kWave * kSumSlices)
refine_backward_sum_kernel(const double *slabs, float *grad_w1, float *grad_b1, int H, int blocks)
{
    __shared__ double s_part[kSumSlices][2][kWave];
    const int lane = threadIdx.x & (kWave - 1), slice = threadIdx.x >> 6;
    const int h = blockIdx.x * kWave + lane;
    double sw = 0.0, sb = 0.0;
    if (h < H) {
        for (int b = slice; b < blocks; b += kSumSlices) {
            sw += slabs[(size_t)b * 2 * H + h];
            sb += slabs[(size_t)b * 2 * H + H + h];
        }
    }
    s_part[slice][0][lane] = sw;
    s_part[slice][1][lane] = sb;
    __syncthreads();
    if (slice == 0 && h < H) {
        for (int q = 1; q < kSumSlices; ++q) {
            sw += s_part[q][0][lane];
            sb += s_part[q][1][lane];
        }
        grad_w1[h] = (float)sw;
        grad_b1[h] = (float)sb;
    }
}

int bwd_tiles(int rows) { return (rows + kRowsPerBlock - 1) / kRowsPerBlock; }
int bwd_blocks(int rows) { return bwd_tiles(rows) < kBwdMaxBlocks ? bwd_tiles(rows) : kBwdMaxBlocks; }
// the fewest passes over h with at most 256 threads, then the fewest whole waves that cover a pass
int bwd_threads(int H)
{
    const int chunks = (H + kBwdMaxThreads - 1) / kBwdMaxThreads;
    const int per = (H + chunks - 1) / chunks;
    return (per + kWave - 1) / kWave * kWave;
}

}  // namespace

hipError_t launch_refine_aggregate(const float *topk16, const float *u_pre, const float *w1,
                                   const float *b1, float *out, float *wsum, int rows, int H,
                                   hipStream_t stream)
{
    const int blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(refine_aggregate_kernel, dim3(blocks), dim3(kRefineThreads), 0, stream, topk16,
                       u_pre, w1, b1, out, wsum, rows, H);
    return hipGetLastError();
}

size_t refine_backward_workspace_bytes(int rows, int H)
{
    if (rows <= 0 || H <= 0) return 0;
    return sizeof(double) * 2 * (size_t)H * (size_t)bwd_blocks(rows);
}

hipError_t launch_refine_backward(const float *topk16, const float *u_pre, const float *w1, const float *b1,
                                  const float *grad_out, const float *grad_wsum, float *grad_u, float *grad_w1,
                                  float *grad_b1, int rows, int H, void *ws, hipStream_t stream)
{
    const int blocks = bwd_blocks(rows);
    double *slabs = static_cast<double *>(ws);
    hipLaunchKernelGGL(refine_backward_kernel, dim3(blocks), dim3(bwd_threads(H)), 0, stream, topk16, u_pre, w1, b1,
                       grad_out, grad_wsum, grad_u, slabs, rows, H, bwd_tiles(rows));
    hipLaunchKernelGGL(refine_backward_sum_kernel, dim3((H + kWave - 1) / kWave), dim3(kWave * kSumSlices), 0, stream,
                       slabs, grad_w1, grad_b1, H, blocks);
    return hipGetLastError();
}

}  // namespace lapwarm
