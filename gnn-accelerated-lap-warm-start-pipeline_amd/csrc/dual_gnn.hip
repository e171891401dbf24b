// dual_gnn.hip -- DualGNN's DualLayer attention without the (B, N, N, hidden) edge embedding.
//
// The attention scores are linear in the edge embedding, so the last Linear(128, hidden) of the edge MLP folds
// into the score weights ("DualGNN"): per edge only 10 -> 128 -> GELU -> 128 -> GELU -> 2 * heads
// remains, and nothing wider than 2 * heads floats per edge reaches HBM.
//
// dual_edge_scores_kernel: a workgroup of 8 waves stages W1, b1, W2, b2 and the folded G in LDS once (W2 rows
// padded to 132 floats: conflict-free 16-byte reads) and walks tiles of 128 edges, 16 per wave.  All three
// products run TRANSPOSED on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain): the weights are the A
// operand (row = output unit), the edges the B operand (column = edge = lane & 15).  A result tile then has its
// edge on the lane and its 4 output units (4 * (lane >> 4) + r) in the 4 accumulator registers, which is exactly
// the B fragment of the next product's k-steps: k-step (t, r) sums over the units 16 t + 4 g + r, g = 0..3, and
// lane group g supplies its own register r.  The A operand reads W[out][16 t + 4 g + r]: one float4 per (m, t).
// No lane movement, no LDS round trip between the layers; GELU (erf form) runs on the VALU in registers.
// 173 VGPRs, no scratch, 83 200 B of LDS: one workgroup per compute unit, two waves per SIMD.
//
// dual_attention_kernel: one workgroup per (16 queries, head, direction, instance), two passes over the keys
// (maximum, then exp / sum / weighted values), fp32, sums in a fixed order: equal inputs give equal bits.
#include "dual_gnn.hpp"

#include <atomic>

namespace lapwarm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEsThreads = 512;
constexpr int kEsWaves = kEsThreads / 64;
constexpr int kEsEdgesPerWave = 16;  // one 16-edge column tile per wave
constexpr int kEsTile = kEsWaves * kEsEdgesPerWave;
constexpr int kHid = kDualEdgeHidden;
constexpr int kWStride = kHid + 4;   // LDS row stride of W2 and G in floats
constexpr int kKPad = 12;            // K = 10 zero-padded to three k-steps of 4
constexpr int kOutPad = 16;          // 2 * heads padded to the tile width
constexpr int kEsLdsFloats = kHid * kWStride + kOutPad * kWStride + kHid * kKPad + 2 * kHid;
constexpr int kEsMaxBlocks = 256;    // one resident workgroup per compute unit (83 KB of LDS each)

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__device__ __forceinline__ f32x4 gelu4(f32x4 v)
{
    f32x4 o;
    o[0] = gelu_erf(v[0]);
    o[1] = gelu_erf(v[1]);
    o[2] = gelu_erf(v[2]);
    o[3] = gelu_erf(v[3]);
    return o;
}

// The staged weights of one workgroup (dynamic LDS, kEsLdsFloats floats).
struct EsWeights {
    const float *W2s;  // [128][132]
    const float *Gs;   // [16][132], rows >= 2 * heads are 0
    const float *W1s;  // [128][12], columns 10, 11 are 0
    const float *b1s;  // [128]
    const float *b2s;  // [128]
};

// All threads of the workgroup; ends with a barrier.
__device__ __forceinline__ EsWeights es_stage_weights(const float *W1, const float *b1, const float *W2,
                                                      const float *b2, const float *G, int outs)
{
    extern __shared__ __align__(16) float es_lds[];
    float *W2s = es_lds;
    float *Gs = W2s + kHid * kWStride;
    float *W1s = Gs + kOutPad * kWStride;
    float *b1s = W1s + kHid * kKPad;
    float *b2s = b1s + kHid;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kHid * kHid; idx += kEsThreads) W2s[(idx >> 7) * kWStride + (idx & 127)] = W2[idx];
    for (int idx = tid; idx < kOutPad * kHid; idx += kEsThreads)
        Gs[(idx >> 7) * kWStride + (idx & 127)] = (idx >> 7) < outs ? G[idx] : 0.0f;
    for (int idx = tid; idx < kHid * kKPad; idx += kEsThreads) {
        const int r = idx / kKPad, c = idx - r * kKPad;
        W1s[idx] = c < kDualEdgeIn ? W1[r * kDualEdgeIn + c] : 0.0f;
    }
    if (tid < kHid) {
        b1s[tid] = b1[tid];
        b2s[tid] = b2[tid];
    }
    __syncthreads();
    return EsWeights{W2s, Gs, W1s, b1s, b2s};
}

// The scores of one wave's 16 edges: f, the edge's features or null for a lane without an edge (read as zeros);
// lane group g = lane >> 4 holds the outputs 4 g + r in register r.  An edge is one column of every product, so its
// scores do not depend on which edges share its tile.
__device__ __forceinline__ f32x4 es_wave_tile(const EsWeights &w, const float *f, int col, int g)
{
    // B fragments of the first product: F^T, k = 4 s + g on the lane group, edge on lane & 15
    float fb[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        fb[s] = (f && k < kDualEdgeIn) ? f[k] : 0.0f;
    }
    f32x4 h1[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b1s[16 * m + 4 * g]);
#pragma unroll
        for (int s = 0; s < 3; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.W1s[(16 * m + col) * kKPad + 4 * s + g], fb[s], acc, 0, 0, 0);
        h1[m] = gelu4(acc);
    }
    // second and third product together: block m of h2 is the k-steps (t = m, r) of the third product, so it
    // is used as soon as it exists.  The loop over m stays rolled (two blocks per trip: two independent
    // accumulator chains); unrolled, the scheduler hoists every LDS read of W2 and spills.
    f32x4 sc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int m = 0; m < 8; ++m) {
        f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b2s[16 * m + 4 * g]);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&w.W2s[(16 * m + col) * kWStride + 16 * t + 4 * g]);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], h1[t][r], acc, 0, 0, 0);
        }
        const f32x4 h2 = gelu4(acc);
        const f32x4 gm = *reinterpret_cast<const f32x4 *>(&w.Gs[col * kWStride + 16 * m + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[r], h2[r], sc, 0, 0, 0);
    }
    return sc;
}

__global__ void __launch_bounds__(kEsThreads)
dual_edge_scores_kernel(const float *F, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *G, float *scores, long long E, long long NN, int heads, long long tiles)
{
    const int outs = 2 * heads;
    const EsWeights w = es_stage_weights(W1, b1, W2, b2, G, outs);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long e = tile * kEsTile + (long long)wave * kEsEdgesPerWave + col;
        const f32x4 sc = es_wave_tile(w, e < E ? F + e * kDualEdgeIn : nullptr, col, g);
        // the tail tile: an edge past the end was read as zeros and is not written
        if (e < E) {
            const long long b = e / NN, rem = e - b * NN;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 4 * g + r;  // dir * heads + h
                if (o < outs) scores[(b * outs + o) * NN + rem] = sc[r];
            }
        }
    }
}

// The batch of different sizes: only the edges (i, j < n_b) of every instance, in the padded layouts.  The unit of
// work is a wave tile, 16 consecutive j of one row i of one instance (the tail of a row is rounded up to a tile, its
// lanes beyond n_b read zeros and write nothing); the wave tiles of all instances are numbered one instance behind
// the other, row by row, and wave w of workgroup g takes the numbers 8 g + w, + 8 gridDim.x, ...  A wave walks the
// instances in order with the running first number of each, so no prefix sum is stored anywhere, and the waves of
// a workgroup share no barrier after the weights are staged.
__global__ void __launch_bounds__(kEsThreads)
dual_edge_scores_ragged_kernel(const float *F, const float *W1, const float *b1, const float *W2, const float *b2,
                               const float *G, float *scores, const int *sizes, int batch, int N, int heads)
{
    const int outs = 2 * heads;
    const EsWeights w = es_stage_weights(W1, b1, W2, b2, G, outs);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const long long stride = (long long)gridDim.x * kEsWaves;
    const size_t NN = (size_t)N * N;
    long long next = (long long)blockIdx.x * kEsWaves + wave, first = 0;
    for (int b = 0; b < batch; ++b) {
        int n = sizes[b];
        n = (n >= 1 && n <= N) ? n : 0;
        const int groups = (n + kEsEdgesPerWave - 1) / kEsEdgesPerWave;
        const long long count = (long long)n * groups;  // at most 16384 * 1024
        for (; next < first + count; next += stride) {
            const int t = (int)(next - first);
            const int i = t / groups, j = (t - i * groups) * kEsEdgesPerWave + col;
            const size_t at = (size_t)i * N + j;
            const f32x4 sc = es_wave_tile(w, j < n ? F + ((size_t)b * NN + at) * kDualEdgeIn : nullptr, col, g);
            if (j < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = 4 * g + r;  // dir * heads + h
                    if (o < outs) scores[((size_t)b * outs + o) * NN + at] = sc[r];
                }
            }
        }
        first += count;
    }
}

constexpr int kAtThreads = 256;
constexpr int kTQ = 16;        // queries per workgroup; 16 threads per query
constexpr int kTK = 64;        // keys per LDS tile
constexpr int kDChunk = 128;   // head_dim columns per pass over the keys: 8 per thread

__device__ __forceinline__ float at_neg_inf() { return __int_as_float(0xff800000); }

__global__ void __launch_bounds__(kAtThreads) dual_attention_kernel(DualAttnParams p)
{
    __shared__ float s_e[kTQ][kTK + 1];
    __shared__ float s_v[kTK][kDChunk];
    __shared__ float s_max[kTQ];
    const int tid = threadIdx.x;
    const int dir = blockIdx.z & 1, b = blockIdx.z >> 1, h = blockIdx.y;
    const int q0 = blockIdx.x * kTQ;
    const int N = p.n, D = p.head_dim, hidden = p.heads * p.head_dim;
    const size_t NN = (size_t)N * N;
    const float *sc = p.scores + (((size_t)b * 2 + dir) * p.heads + h) * NN;
    const float *a = (dir ? p.a_col : p.a_row) + ((size_t)b * p.heads + h) * N;
    const float *c = (dir ? p.c_col : p.c_row) + ((size_t)b * p.heads + h) * N;
    const float *val = (dir ? p.row_val : p.col_val) + (size_t)b * N * hidden + (size_t)h * D;
    float *msg = (dir ? p.col_msg : p.row_msg) + (size_t)b * N * hidden + (size_t)h * D;
    // with sizes the mask is the prefix: nb bounds the queries and the keys, and `mask` is not read
    int nb = N;
    if (p.sizes) {
        nb = p.sizes[b];
        nb = (nb >= 1 && nb <= N) ? nb : 0;
    }
    const unsigned char *mask = (p.mask && !p.sizes) ? p.mask + (size_t)b * N : nullptr;
    const int cq = tid >> 4, slot = tid & 15;
    if (q0 >= nb) {  // a block of padded queries (workgroup-uniform): zero messages, no key is read
        for (int idx = tid; idx < kTQ * D; idx += kAtThreads) {
            const int q = q0 + idx / D;
            if (q < N) msg[(size_t)q * hidden + idx % D] = 0.0f;
        }
        return;
    }
    const float kb = p.kbias[dir * p.heads + h];

    // the tile s_e[q][k] of leaky_relu scores (pass 0) or of exp(score - max) (pass 1).  Loads run along the
    // contiguous index of scores: the key for the row direction, the query for the column direction.
    auto load_tile = [&](int k0, bool exps) {
#pragma unroll
        for (int r = 0; r < (kTQ * kTK) / kAtThreads; ++r) {
            const int lq = dir ? (tid & 15) : ((tid >> 6) + 4 * r);
            const int lk = dir ? ((tid >> 4) + 16 * r) : (tid & 63);
            const int q = q0 + lq, k = k0 + lk;
            float s = at_neg_inf();
            if (q < nb && k < nb && (!mask || (mask[q] && mask[k]))) {
                const size_t at = dir ? (size_t)k * N + q : (size_t)q * N + k;
                s = ((a[q] + c[k]) + sc[at]) + kb;
                s = s >= 0.0f ? s : 0.2f * s;
            }
            if (exps) s = (s == at_neg_inf()) ? 0.0f : expf(s - s_max[lq]);
            s_e[lq][lk] = s;
        }
    };

    float m = at_neg_inf();
    for (int k0 = 0; k0 < nb; k0 += kTK) {  // up to the last tile that holds a key of the prefix
        load_tile(k0, false);
        __syncthreads();
#pragma unroll
        for (int k = slot; k < kTK; k += 16) m = fmaxf(m, s_e[cq][k]);
        __syncthreads();
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 16));
    if (slot == 0) s_max[cq] = m;
    __syncthreads();

    for (int d0 = 0; d0 < D; d0 += kDChunk) {
        const int dlen = (D - d0) < kDChunk ? (D - d0) : kDChunk;
        float acc[kDChunk / 16];
#pragma unroll
        for (int r = 0; r < kDChunk / 16; ++r) acc[r] = 0.0f;
        float sum = 0.0f;
        for (int k0 = 0; k0 < nb; k0 += kTK) {
            load_tile(k0, true);
            for (int idx = tid; idx < kTK * dlen; idx += kAtThreads) {
                const int k = idx / dlen, d = idx - k * dlen;
                s_v[k][d] = (k0 + k < nb) ? val[(size_t)(k0 + k) * hidden + d0 + d] : 0.0f;
            }
            __syncthreads();
            for (int k = 0; k < kTK; ++k) {
                const float e = s_e[cq][k];
                sum += e;
#pragma unroll
                for (int r = 0; r < kDChunk / 16; ++r) {
                    const int d = slot + 16 * r;
                    if (d < dlen) acc[r] += e * s_v[k][d];
                }
            }
            __syncthreads();
        }
        const int q = q0 + cq;
        if (q < N) {
#pragma unroll
            for (int r = 0; r < kDChunk / 16; ++r) {
                const int d = slot + 16 * r;
                if (d < dlen) msg[(size_t)q * hidden + d0 + d] = sum > 0.0f ? acc[r] / sum : 0.0f;
            }
        }
    }
}

constexpr size_t kEsLdsBytes = (size_t)kEsLdsFloats * sizeof(float);

// more dynamic LDS than the 64 KB default is allowed once per process and kernel, not on each of a forward's
// launches (and not inside a capture: the first launch is the uncaptured warm-up every captured call has)
hipError_t es_raise_lds(const void *kernel, std::atomic<bool> &raised)
{
    if (!raised.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEsLdsBytes);
        if (e != hipSuccess) return e;
        raised.store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

size_t dual_gnn_workspace_bytes(int batch, int n, int heads)
{
    if (batch < 1 || batch > kDualMaxBatch || n < 1 || n > 16384 || heads < 1 || heads > kDualMaxHeads) return 0;
    const size_t bytes = (size_t)batch * 2 * heads * n * n * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

hipError_t launch_dual_edge_scores(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                   const float *b2, const float *G, float *scores, int batch, int n, int heads,
                                   hipStream_t stream)
{
    const long long NN = (long long)n * n, E = NN * batch;
    const long long tiles = (E + kEsTile - 1) / kEsTile;
    const int blocks = (int)(tiles < kEsMaxBlocks ? tiles : kEsMaxBlocks);
    static std::atomic<bool> raised{false};
    if (hipError_t e = es_raise_lds(reinterpret_cast<const void *>(dual_edge_scores_kernel), raised)) return e;
    hipLaunchKernelGGL(dual_edge_scores_kernel, dim3(blocks), dim3(kEsThreads), kEsLdsBytes, stream, edge_feat, W1,
                       b1, W2, b2, G, scores, E, NN, heads, tiles);
    return hipGetLastError();
}

hipError_t launch_dual_edge_scores_ragged(const float *edge_feat, const float *W1, const float *b1, const float *W2,
                                          const float *b2, const float *G, float *scores, const int *sizes, int batch,
                                          int n, int heads, hipStream_t stream)
{
    // the sizes are on the device: the grid is sized for the padded batch, and a workgroup without a tile leaves
    const long long wave_tiles = (long long)batch * n * ((n + kEsEdgesPerWave - 1) / kEsEdgesPerWave);
    const long long tiles = (wave_tiles + kEsWaves - 1) / kEsWaves;
    const int blocks = (int)(tiles < kEsMaxBlocks ? tiles : kEsMaxBlocks);
    static std::atomic<bool> raised{false};
    if (hipError_t e = es_raise_lds(reinterpret_cast<const void *>(dual_edge_scores_ragged_kernel), raised)) return e;
    hipLaunchKernelGGL(dual_edge_scores_ragged_kernel, dim3(blocks), dim3(kEsThreads), kEsLdsBytes, stream, edge_feat,
                       W1, b1, W2, b2, G, scores, sizes, batch, n, heads);
    return hipGetLastError();
}

hipError_t launch_dual_attention(const DualAttnParams &p, hipStream_t stream)
{
    const dim3 grid((p.n + kTQ - 1) / kTQ, p.heads, 2 * p.batch);
    hipLaunchKernelGGL(dual_attention_kernel, grid, dim3(kAtThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace lapwarm
