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
// (maximum, then exp / sum / weighted values), fp32, sums in a fixed order: equal inputs give equal bits.  With the
// two statistics pointers set it also leaves every query's maximum and sum for the backward.
//
// The backward ("DualGNN backward"), no atomics anywhere, no kernel with scratch:
//   dual_attention_bwd_query_kernel  90 VGPRs, 49 664 B LDS, 3 waves/SIMD   dS, da, fp64 partials of dkb
//   dual_attention_bwd_key_kernel    88 VGPRs, 41 088 B LDS, 3 waves/SIMD   dc, dval
//   dual_attention_bwd_kbias_kernel  the partials in order, fp64
//   dual_edge_backward_kernel        224 VGPRs, 83 200 B LDS (through es_raise_lds), 2 waves/SIMD: the recompute
//                                    of a chunk of edges and the way back through it, rows into the workspace
//   dual_edge_wgrad_kernel           61 VGPRs, no LDS, 8 waves/SIMD: the five sums over edges as TN MFMA products
//   dual_edge_wgrad_reduce_kernel    workgroups and chunks in order, fp64, rounded once
//
// Dropout inside the fused region (dual_dropout.hpp; DESIGN.md, "DualGNN backward"): every kernel that sees h1 or an
// attention weight is a template <bool DROP>.  The figures above are those of DROP = false, whose code is unchanged;
// DROP = true regenerates the mask from (seed, stream, element index) wherever it is needed, stores none, and takes
// 227 (edge scores), 244 (ragged), 102 (attention), 101 / 108 (backward query / key) and 244 (edge backward) VGPRs
// with the same LDS, no scratch and the same waves per SIMD (profiles/dual_gnn_dropout.md).
//
// The bf16 edge MLP (second template parameter BF16 of the edge kernels; contract and layout below, DESIGN.md "DualGNN
// bf16 edge MLP").  A kernel stages EsWeights or EsWeightsBf (es_stage_weights, picked by std::bool_constant<BF16>), and
// the staged type picks the tile: es_wave_tile and eb_wave_tile are two overloads each, sharing es_first_pre /
// es_first_layer / es_second_layer (fp32) and es_first_pre / bf_first_layer / bf_second_layer (bf16) between forward
// and backward.  BF16 = false is the code and the figures above.  BF16 = true, no scratch anywhere:
//   dual_edge_scores_kernel          152 VGPRs (DROP: 202), 44 288 B LDS, one workgroup of 8 waves per CU: 2 waves/SIMD
//   dual_edge_scores_ragged_kernel   161 VGPRs (DROP: 212), 44 288 B LDS, 2 waves/SIMD
//   dual_edge_backward_kernel        187 VGPRs (DROP: 235), 91 392 B LDS (W2 and W2^T staged, 8 KB of flush buffers),
//                                    2 waves/SIMD
//   dual_edge_wgrad_bf16_kernel      94 VGPRs, no LDS, 5 waves/SIMD
// Staged in bf16 the forward's weights would let two workgroups share a CU's LDS, but not at 152 VGPRs; that and
// 16-edge tiles at higher occupancy are not measured yet (profiles/dual_gnn_bf16.md).
//
// Written once and shared: the wave tiles of an instance (es_instance_tiles, host and device), the clamped prefix
// (dual_prefix_len), the attention kernels' tile slot (at_tile_slot) and their (b, dir, h) view (AtView, AtBwdView), the
// slice and store of stage 2 (wg_begin, wg_store).  The host takes one record per call (DualEdgeParams, DualEdgeGrads,
// DualAttnParams), picks an instantiation with dispatch_bools, and keeps the raised-LDS flag per kernel
// (es_raise_lds<Kernel>).  Figures of this build beside its parent's: profiles/dual_gnn_refactor.md.
#include "dual_gnn.hpp"

#include <atomic>
#include <type_traits>

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

// The wave tiles of one instance of a padded batch: 16 consecutive j of one row i, a row's tail rounded up to a tile.
// A size outside 1..N is an empty instance.  The kernels and the host's workspace layout number the tiles from here.
__host__ __device__ __forceinline__ int dual_prefix_len(int size, int N) { return (size >= 1 && size <= N) ? size : 0; }

struct EsInstanceTiles {
    int n, groups;    // the clamped size; tiles per row
    long long count;  // at most 16384 * 1024
};

__host__ __device__ __forceinline__ EsInstanceTiles es_instance_tiles(int size, int N)
{
    const int n = dual_prefix_len(size, N);
    const int groups = (n + kEsEdgesPerWave - 1) / kEsEdgesPerWave;
    return EsInstanceTiles{n, groups, (long long)n * groups};
}

// The staged weights of one workgroup (dynamic LDS, kEsLdsFloats floats).  Row and kDsRegs: what the backward's tile
// writes per edge and how many dS values of its edge a lane holds.
struct EsWeights {
    typedef float Row;
    static constexpr int kDsRegs = 4;
    const float *W2s;  // [128][132]
    const float *Gs;   // [16][132], rows >= 2 * heads are 0
    const float *W1s;  // [128][12], columns 10, 11 are 0
    const float *b1s;  // [128]
    const float *b2s;  // [128]
};

// All threads of the workgroup; ends with a barrier.  The tag picks the fp32 images (here) or the bf16 ones (below);
// BWD: the fp32 backward reads the forward's images.
template <bool BWD>
__device__ __forceinline__ EsWeights es_stage_weights(std::false_type, const float *W1, const float *b1, const float *W2,
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

__device__ __forceinline__ f32x4 es_drop4(f32x4 v, unsigned bits, int t, float scale);

// B fragments of the first product: F^T, k = 4 s + g on the lane group, edge on lane & 15; f null: zeros
__device__ __forceinline__ void es_feature_fragment(const float *f, int g, float (&fb)[3])
{
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        fb[s] = (f && k < kDualEdgeIn) ? f[k] : 0.0f;
    }
}

// x1 = W1 f + b1 of block m: three k-steps
__device__ __forceinline__ f32x4 es_first_pre(const EsWeights &w, const float (&fb)[3], int m, int col, int g)
{
    f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b1s[16 * m + 4 * g]);
#pragma unroll
    for (int s = 0; s < 3; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.W1s[(16 * m + col) * kKPad + 4 * s + g], fb[s], acc, 0, 0, 0);
    return acc;
}

// block m of h1 = GELU(x1), dropped with DROP
template <bool DROP>
__device__ __forceinline__ f32x4 es_first_layer(const EsWeights &w, const float (&fb)[3], int m, int col, int g,
                                                unsigned keep, float scale)
{
    const f32x4 h1 = gelu4(es_first_pre(w, fb, m, col, g));
    if constexpr (DROP) return es_drop4(h1, keep, m, scale);
    return h1;
}

// x2 of block m: the k-steps (t, r) over h1
__device__ __forceinline__ f32x4 es_second_layer(const EsWeights &w, const f32x4 (&h1)[8], int m, int col, int g)
{
    f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b2s[16 * m + 4 * g]);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(&w.W2s[(16 * m + col) * kWStride + 16 * t + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], h1[t][r], acc, 0, 0, 0);
    }
    return acc;
}

// ---- the bf16 edge MLP (BF16 = true; DESIGN.md, "DualGNN bf16 edge MLP") ------------------------------------------
// The contract: round-to-nearest-even from fp32 to bf16 (v_cvt_pk_bf16_f32, which the compiler emits for a cast) of
// edge_feat when a lane loads it, of W1, W2 and G when they are staged, of h1 after GELU and dropout, of h2 after
// GELU, and in the backward of dS, dh2pre, dh1pre and the column of ones where they become MFMA operands.  b1, b2,
// the pre-activations (fp32 accumulators of v_mfma_f32_16x16x32_bf16), GELU, GELU', the score and every gradient sum
// stay fp32 (fp64 across workgroups and chunks).  The transposed arrangement of the fp32 form carries over: a result
// tile has its edge on the lane and the units 4 g + r of a 16-unit block in register r, and one k-step of 32 covers
// the blocks 2 s and 2 s + 1, lane group g supplying its own eight values 32 s + 4 g + r and 32 s + 16 + 4 g + r.
// The weights are staged with their k index permuted to match (es_kpos), so an A fragment is one 16-byte LDS read;
// a permutation of k applied to both operands changes no product.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kBfStride = kHid + 8;        // LDS row stride of W2, W2^T and G in bf16: 272 B, conflict-free b128 reads
constexpr int kBfK1 = 16;                  // K = 10 (and the 2 * heads of G^T) padded to 16; k 16..31 are zero lanes
constexpr int kBfFlushUnits = 32;          // the backward's transpose buffer: 32 units x 16 edges per wave
constexpr size_t kEsBfFwdBytes = (size_t)(kHid * kBfStride + kOutPad * kBfStride + kHid * kBfK1) * 2 + 2 * kHid * 4;
constexpr size_t kEsBfBwdBytes =
    kEsBfFwdBytes + (size_t)(kHid * kBfStride + kHid * kBfK1 + kEsWaves * kBfFlushUnits * kEsEdgesPerWave) * 2;

// where unit u of a 128-wide k index lies in a staged row: k-step u >> 5, then lane group, block parity, register
__device__ __forceinline__ int es_kpos(int u) { return (u & ~31) | (((u >> 2) & 3) << 3) | (((u >> 4) & 1) << 2) | (u & 3); }

struct EsWeightsBf {
    typedef __bf16 Row;  // per wave tile an image [544 units][16 edges]
    static constexpr int kDsRegs = 8;
    const __bf16 *W2s;   // [128][136], k permuted by es_kpos
    const __bf16 *Gs;    // [16][136], k permuted, rows >= 2 * heads are 0
    const __bf16 *W1s;   // [128][16], columns >= 10 are 0
    const float *b1s;    // [128]
    const float *b2s;    // [128]
    // the backward only
    const __bf16 *W2Ts;  // [128][136]: W2Ts[k][es_kpos(o)] = W2[o][k]
    const __bf16 *GTs;   // [128][16]: GTs[k][o] = G[o][k], columns >= 2 * heads are 0
    __bf16 *flush;       // [8 waves][32 units][16 edges]
};

// All threads of the workgroup; ends with a barrier.  BWD: the transposes and the flush buffers as well.
template <bool BWD>
__device__ __forceinline__ EsWeightsBf es_stage_weights(std::true_type, const float *W1, const float *b1, const float *W2,
                                                        const float *b2, const float *G, int outs)
{
    extern __shared__ __align__(16) float es_lds[];
    __bf16 *W2s = reinterpret_cast<__bf16 *>(es_lds);
    __bf16 *Gs = W2s + kHid * kBfStride;
    __bf16 *W1s = Gs + kOutPad * kBfStride;
    float *b1s = reinterpret_cast<float *>(W1s + kHid * kBfK1);
    float *b2s = b1s + kHid;
    __bf16 *W2Ts = reinterpret_cast<__bf16 *>(b2s + kHid);
    __bf16 *GTs = W2Ts + kHid * kBfStride;
    __bf16 *flush = GTs + kHid * kBfK1;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kHid * kHid; idx += kEsThreads) {
        const int o = idx >> 7, k = idx & 127;
        const __bf16 v = (__bf16)W2[idx];
        W2s[o * kBfStride + es_kpos(k)] = v;
        if constexpr (BWD) W2Ts[k * kBfStride + es_kpos(o)] = v;
    }
    for (int idx = tid; idx < kOutPad * kHid; idx += kEsThreads) {
        const int o = idx >> 7, k = idx & 127;
        const __bf16 v = (__bf16)(o < outs ? G[idx] : 0.0f);
        Gs[o * kBfStride + es_kpos(k)] = v;
        if constexpr (BWD) GTs[k * kBfK1 + o] = v;
    }
    for (int idx = tid; idx < kHid * kBfK1; idx += kEsThreads) {
        const int r = idx >> 4, c = idx & 15;
        W1s[idx] = (__bf16)(c < kDualEdgeIn ? W1[r * kDualEdgeIn + c] : 0.0f);
    }
    if (tid < kHid) {
        b1s[tid] = b1[tid];
        b2s[tid] = b2[tid];
    }
    __syncthreads();
    return EsWeightsBf{W2s, Gs, W1s, b1s, b2s, W2Ts, GTs, flush + (tid >> 6) * kBfFlushUnits * kEsEdgesPerWave};
}

__device__ __forceinline__ bf16x8 bf_zero8()
{
    const __bf16 z = (__bf16)0.0f;
    return bf16x8{z, z, z, z, z, z, z, z};
}

// two accumulator blocks, 2 s and 2 s + 1, as the fragment of k-step s
__device__ __forceinline__ bf16x8 bf_pack(f32x4 lo, f32x4 hi)
{
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3],
                  (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

// 16 k values of a [rows][16] image for the lane groups 0 and 1; the groups 2 and 3 hold the zero half of the k-step
__device__ __forceinline__ bf16x8 bf_k16_fragment(const __bf16 *row16, int g)
{
    return g < 2 ? *reinterpret_cast<const bf16x8 *>(row16 + 8 * g) : bf_zero8();
}

// B fragment of the first product: the lane's features k = 8 g + j, rounded as they are loaded
__device__ __forceinline__ bf16x8 bf_feature_fragment(const float *f, int g)
{
    bf16x8 fb = bf_zero8();
    if (f && g < 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (8 * g + j < kDualEdgeIn) fb[j] = (__bf16)f[8 * g + j];
    }
    return fb;
}

// x1 = W1 f + b1 of block m: one k-step
__device__ __forceinline__ f32x4 es_first_pre(const EsWeightsBf &w, bf16x8 fb, int m, int col, int g)
{
    const f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b1s[16 * m + 4 * g]);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf_k16_fragment(&w.W1s[(16 * m + col) * kBfK1], g), fb, acc, 0, 0, 0);
}

// h1 of the lane's edge as the four k-step fragments of the second product (rounded after GELU and dropout)
template <bool DROP>
__device__ __forceinline__ void bf_first_layer(const EsWeightsBf &w, bf16x8 fb, int col, int g, unsigned keep,
                                               float scale, bf16x8 (&h1)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        f32x4 blk[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int m = 2 * s + half;
            blk[half] = gelu4(es_first_pre(w, fb, m, col, g));
            if constexpr (DROP) blk[half] = es_drop4(blk[half], keep, m, scale);
        }
        h1[s] = bf_pack(blk[0], blk[1]);
    }
}

// x2 of block m: four k-steps over h1
__device__ __forceinline__ f32x4 bf_second_layer(const EsWeightsBf &w, const bf16x8 (&h1)[4], int m, int col, int g)
{
    f32x4 acc = *reinterpret_cast<const f32x4 *>(&w.b2s[16 * m + 4 * g]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *reinterpret_cast<const bf16x8 *>(&w.W2s[(16 * m + col) * kBfStride + 32 * s + 8 * g]), h1[s], acc, 0, 0, 0);
    return acc;
}

// The keep bits of a lane's edge (dual_dropout.hpp, stream 0): the lane holds the units 16 t + 4 g + r of its edge,
// the group 4 t + g of four consecutive units, so one Philox call gives the four registers of a (t, g).  Bit 4 t + r
// is the keep flag of h1[t][r].  `edge` is the edge's index (b N + i) N + j in the padded layout.
__device__ __forceinline__ unsigned es_keep_bits(const DualDropout &d, unsigned long long edge, int g)
{
    unsigned bits = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        unsigned wd[4];
        dual_dropout_words(d.k0, d.k1, kDropStreamEdge, edge * (kHid / 4) + 4 * t + g, wd);
#pragma unroll
        for (int r = 0; r < 4; ++r) bits |= (wd[r] >= d.threshold ? 1u : 0u) << (4 * t + r);
    }
    return bits;
}

// keep * scale * h1 for block t of a lane's h1
__device__ __forceinline__ f32x4 es_drop4(f32x4 v, unsigned bits, int t, float scale)
{
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = ((bits >> (4 * t + r)) & 1u) ? v[r] * scale : 0.0f;
    return o;
}

// The scores of one wave's 16 edges: f, the edge's features or null for a lane without an edge (read as zeros);
// lane group g = lane >> 4 holds the outputs 4 g + r in register r.  An edge is one column of every product, so its
// scores do not depend on which edges share its tile.  DROP: h1 is keep * scale * h1, `keep` from es_keep_bits.
// The staged weights' type picks the tile: fp32 here, bf16 below.
template <bool DROP>
__device__ __forceinline__ f32x4 es_wave_tile(const EsWeights &w, const float *f, int col, int g, unsigned keep = 0,
                                              float scale = 1.0f)
{
    float fb[3];
    es_feature_fragment(f, g, fb);
    f32x4 h1[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) h1[m] = es_first_layer<DROP>(w, fb, m, col, g, keep, scale);
    // second and third product together: block m of h2 is the k-steps (t = m, r) of the third product, so it
    // is used as soon as it exists.  The loop over m stays rolled (two blocks per trip: two independent
    // accumulator chains); unrolled, the scheduler hoists every LDS read of W2 and spills.
    f32x4 sc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int m = 0; m < 8; ++m) {
        const f32x4 h2 = gelu4(es_second_layer(w, h1, m, col, g));
        const f32x4 gm = *reinterpret_cast<const f32x4 *>(&w.Gs[col * kWStride + 16 * m + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[r], h2[r], sc, 0, 0, 0);
    }
    return sc;
}

// The same tile on v_mfma_f32_16x16x32_bf16 (the contract above): 8 + 32 + 4 MFMAs for 16 edges.
template <bool DROP>
__device__ __forceinline__ f32x4 es_wave_tile(const EsWeightsBf &w, const float *f, int col, int g, unsigned keep = 0,
                                              float scale = 1.0f)
{
    bf16x8 h1[4];
    bf_first_layer<DROP>(w, bf_feature_fragment(f, g), col, g, keep, scale, h1);
    f32x4 sc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {  // two blocks of h2 are k-step s of the third product
        const f32x4 lo = gelu4(bf_second_layer(w, h1, 2 * s, col, g));
        const f32x4 hi = gelu4(bf_second_layer(w, h1, 2 * s + 1, col, g));
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *reinterpret_cast<const bf16x8 *>(&w.Gs[col * kBfStride + 32 * s + 8 * g]), bf_pack(lo, hi), sc, 0, 0, 0);
    }
    return sc;
}

template <bool DROP, bool BF16>
__global__ void __launch_bounds__(kEsThreads)
dual_edge_scores_kernel(const float *F, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *G, float *scores, long long E, long long NN, int heads, long long tiles,
                        DualDropout drop)
{
    const int outs = 2 * heads;
    const auto w = es_stage_weights<false>(std::bool_constant<BF16>{}, W1, b1, W2, b2, G, outs);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long e = tile * kEsTile + (long long)wave * kEsEdgesPerWave + col;
        // the keep bits before the MFMA chain, while few registers are live
        const unsigned keep = DROP ? es_keep_bits(drop, (unsigned long long)e, g) : 0u;
        const f32x4 sc = es_wave_tile<DROP>(w, e < E ? F + e * kDualEdgeIn : nullptr, col, g, keep, drop.scale);
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
template <bool DROP, bool BF16>
__global__ void __launch_bounds__(kEsThreads)
dual_edge_scores_ragged_kernel(const float *F, const float *W1, const float *b1, const float *W2, const float *b2,
                               const float *G, float *scores, const int *sizes, int batch, int N, int heads,
                               DualDropout drop)
{
    const int outs = 2 * heads;
    const auto w = es_stage_weights<false>(std::bool_constant<BF16>{}, W1, b1, W2, b2, G, outs);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const long long stride = (long long)gridDim.x * kEsWaves;
    const size_t NN = (size_t)N * N;
    long long next = (long long)blockIdx.x * kEsWaves + wave, first = 0;
    for (int b = 0; b < batch; ++b) {
        const EsInstanceTiles it = es_instance_tiles(sizes[b], N);
        for (; next < first + it.count; next += stride) {
            const int t = (int)(next - first);
            const int i = t / it.groups, j = (t - i * it.groups) * kEsEdgesPerWave + col;
            const size_t at = (size_t)i * N + j;
            const unsigned keep = DROP ? es_keep_bits(drop, (unsigned long long)b * NN + at, g) : 0u;
            const f32x4 sc = es_wave_tile<DROP>(w, j < it.n ? F + ((size_t)b * NN + at) * kDualEdgeIn : nullptr, col, g,
                                                keep, drop.scale);
            if (j < it.n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = 4 * g + r;  // dir * heads + h
                    if (o < outs) scores[((size_t)b * outs + o) * NN + at] = sc[r];
                }
            }
        }
        first += it.count;
    }
}

constexpr int kAtThreads = 256;
constexpr int kTQ = 16;        // queries per workgroup; 16 threads per query
constexpr int kTK = 64;        // keys per LDS tile
constexpr int kDChunk = 128;   // head_dim columns per pass over the keys: 8 per thread

__device__ __forceinline__ float at_neg_inf() { return __int_as_float(0xff800000); }

// The index of (b, dir, h, query 0, key 0) in the logical tensor of the attention weights (dual_dropout.hpp, stream 1)
__device__ __forceinline__ unsigned long long at_drop_base(int b, int dir, int h, int heads, int N)
{
    return (unsigned long long)(((size_t)b * 2 + dir) * heads + h) * N * N;
}

// The slot (lq, lk) of a 16 x 64 tile that thread tid moves in round r.  Consecutive threads run along the contiguous
// index of the scores: the key for the row direction, the query for the column direction.  The key-major kernel, whose
// tiles are 16 keys x 64 queries, asks with !dir and swaps the two.
struct AtSlot {
    int lq, lk;
};

__device__ __forceinline__ AtSlot at_tile_slot(int tid, int dir, int r)
{
    return AtSlot{dir ? (tid & 15) : ((tid >> 6) + 4 * r), dir ? ((tid >> 4) + 16 * r) : (tid & 63)};
}

// What the forward and both backward kernels take from the forward's parameters for their (b, dir, h).  bh and node:
// where (b, h) lies in a [batch][heads] tensor and (b, node 0, h, 0) in a [batch][n][heads * head_dim] one.
struct AtView {
    const float *sc, *a, *c, *val;
    const unsigned char *mask;  // null with sizes: the mask is then the prefix [0, nb)
    int nb;                     // bounds the queries and the keys
    size_t bh, node;
};

__device__ __forceinline__ AtView at_view(const DualAttnParams &f, int b, int dir, int h)
{
    const int N = f.n, D = f.head_dim, hidden = f.heads * D;
    AtView v;
    v.bh = (size_t)b * f.heads + h;
    v.node = (size_t)b * N * hidden + (size_t)h * D;
    v.sc = f.scores + (((size_t)b * 2 + dir) * f.heads + h) * ((size_t)N * N);
    v.a = (dir ? f.a_col : f.a_row) + v.bh * N;
    v.c = (dir ? f.c_col : f.c_row) + v.bh * N;
    v.val = (dir ? f.row_val : f.col_val) + v.node;
    v.nb = f.sizes ? dual_prefix_len(f.sizes[b], N) : N;
    v.mask = (f.mask && !f.sizes) ? f.mask + (size_t)b * N : nullptr;
    return v;
}

// DROP: the tile of exp(score - max) carries the keep flag of its (query, key) in the sign bit (an exp is never
// negative): -e is a dropped weight.  The sum takes |e|, the weighted values e * scale or 0, so the statistics are
// those of the undropped softmax and LDS holds what it held.  The flag is a function of (q, k) alone: every pass over
// the keys (head_dim > 128) sees the same mask.
template <bool DROP>
__global__ void __launch_bounds__(kAtThreads) dual_attention_kernel(DualAttnParams p)
{
    __shared__ float s_e[kTQ][kTK + 1];
    __shared__ float s_v[kTK][kDChunk];
    __shared__ float s_max[kTQ];
    const int tid = threadIdx.x;
    const int dir = blockIdx.z & 1, b = blockIdx.z >> 1, h = blockIdx.y;
    const int q0 = blockIdx.x * kTQ;
    const int N = p.n, D = p.head_dim, hidden = p.heads * p.head_dim;
    const AtView v = at_view(p, b, dir, h);
    const float *sc = v.sc, *a = v.a, *c = v.c, *val = v.val;
    const unsigned char *mask = v.mask;
    const int nb = v.nb;
    float *msg = (dir ? p.col_msg : p.row_msg) + v.node;
    const int cq = tid >> 4, slot = tid & 15;
    float *stats = dir ? p.col_stats : p.row_stats;  // the training forward keeps every query's maximum and sum
    if (stats) stats += v.bh * N * 2;
    if (q0 >= nb) {  // a block of padded queries (workgroup-uniform): zero messages, no key is read
        for (int idx = tid; idx < kTQ * D; idx += kAtThreads) {
            const int q = q0 + idx / D;
            if (q < N) msg[(size_t)q * hidden + idx % D] = 0.0f;
        }
        if (stats && tid < 2 * kTQ && q0 + (tid >> 1) < N) stats[(size_t)q0 * 2 + tid] = 0.0f;
        return;
    }
    const float kb = p.kbias[dir * p.heads + h];
    const unsigned long long drop_base = DROP ? at_drop_base(b, dir, h, p.heads, N) : 0;

    // the tile s_e[q][k] of leaky_relu scores (pass 0) or of exp(score - max) (pass 1).  Loads run along the
    // contiguous index of scores: the key for the row direction, the query for the column direction.
    auto load_tile = [&](int k0, bool exps) {
#pragma unroll
        for (int r = 0; r < (kTQ * kTK) / kAtThreads; ++r) {
            const auto [lq, lk] = at_tile_slot(tid, dir, r);
            const int q = q0 + lq, k = k0 + lk;
            float s = at_neg_inf();
            if (q < nb && k < nb && (!mask || (mask[q] && mask[k]))) {
                const size_t at = dir ? (size_t)k * N + q : (size_t)q * N + k;
                s = ((a[q] + c[k]) + sc[at]) + kb;
                s = s >= 0.0f ? s : 0.2f * s;
            }
            if (exps) s = (s == at_neg_inf()) ? 0.0f : expf(s - s_max[lq]);
            if constexpr (DROP) {
                if (exps && !dual_dropout_keep(p.drop, kDropStreamAttn, drop_base + (size_t)q * N + k)) s = -s;
            }
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
                float e = s_e[cq][k];
                if constexpr (DROP) {
                    sum += fabsf(e);
                    e = (__float_as_uint(e) >> 31) ? 0.0f : e * p.drop.scale;
                } else {
                    sum += e;
                }
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
            if (stats && d0 == 0 && slot == 0) {  // a masked query: (-inf, 0), which the backward never uses
                stats[(size_t)q * 2] = s_max[cq];
                stats[(size_t)q * 2 + 1] = sum;
            }
        }
    }
}

// ---- the backward of the attention -----------------------------------------------------------------------------
// With z = ((a[q] + c[k]) + S) + kb, s = leaky_relu(z), w = exp(s - max_q) / sum_q from the forward's statistics:
//   dz[q,k] = w (dw[q,k] - delta[q]) (z >= 0 ? 1 : 0.2), dw = dmsg[q] . val[k], delta = dmsg[q] . msg[q] formed as
//   sum_k w dw (a first pass over the keys that also parks dw in dS); exactly 0 on a masked pair.
// Every sum runs in a fixed order in fp32 (the parts of dkb in fp64); there is no atomic.

struct AtBwdView : AtView {  // and what both backward passes add for their (b, dir, h)
    const float *dmsg, *stats;
    float kb;
};

__device__ __forceinline__ AtBwdView at_bwd_view(const DualAttnBwdParams &p, int b, int dir, int h)
{
    const DualAttnParams &f = p.fwd;
    AtBwdView v{at_view(f, b, dir, h)};
    v.dmsg = (dir ? p.d_col_msg : p.d_row_msg) + v.node;
    v.stats = (dir ? f.col_stats : f.row_stats) + v.bh * f.n * 2;
    v.kb = f.kbias[dir * f.heads + h];
    return v;
}

constexpr int kBwVStride = kDChunk + 1;  // a thread reads the rows slot + 16 r of one column: odd stride, no conflict

// Query-major: one workgroup per (16 queries, head, direction, instance) walks the key tiles; dS, da and the
// workgroup's part of dkb.  The tile of z is loaded, and the tile of dz stored, along the contiguous index of the
// scores as the forward's load_tile does; thread (cq, slot) owns the keys slot + 16 r of query cq in between.
// DROP: dw[q,k] = keep * scale * (dmsg[q] . val[k]), the mask of the forward regenerated; delta = sum_k w dw is then
// dmsg[q] . msg[q] with msg the dropped message, and dz = w (dw - delta) slope as without dropout.
template <bool DROP>
__global__ void __launch_bounds__(kAtThreads) dual_attention_bwd_query_kernel(DualAttnBwdParams p)
{
    __shared__ float s_z[kTQ][kTK + 1];
    __shared__ float s_v[kTK][kBwVStride];
    __shared__ float s_dm[kTQ][kDChunk];
    __shared__ float s_g[kTQ][kTK + 1];
    __shared__ double s_dk[kTQ];
    const int tid = threadIdx.x;
    const int dir = blockIdx.z & 1, b = blockIdx.z >> 1, h = blockIdx.y;
    const int q0 = blockIdx.x * kTQ;
    const int N = p.fwd.n, D = p.fwd.head_dim, heads = p.fwd.heads, hidden = heads * D;
    const AtBwdView v = at_bwd_view(p, b, dir, h);
    const int nb = v.nb;
    float *dS = p.dS + (((size_t)b * 2 + dir) * heads + h) * (size_t)N * N;
    float *da = (dir ? p.da_col : p.da_row) + v.bh * N;
    double *part = p.partials + ((size_t)blockIdx.z * heads + h) * gridDim.x + blockIdx.x;
    const int cq = tid >> 4, slot = tid & 15;
    if (q0 >= nb) {  // padded queries: zero gradients, no score and no dS entry is touched
        if (tid < kTQ && q0 + tid < N) da[q0 + tid] = 0.0f;
        if (tid == 0) *part = 0.0;
        return;
    }
    const int q = q0 + cq;
    const unsigned long long drop_base = DROP ? at_drop_base(b, dir, h, heads, N) : 0;
    const bool live = q < nb && (!v.mask || v.mask[q]);
    float mq = 0.0f, sq = 1.0f;
    if (live) {
        mq = v.stats[(size_t)q * 2];
        sq = v.stats[(size_t)q * 2 + 1];
    }
    // the tile of z (and of what dS holds at the same places) in the load_tile mapping of the forward; a thread
    // loads and stores the same places in both passes, so its own program order is all the passes need
    auto load_z = [&](int k0, bool with_dw) {
#pragma unroll
        for (int r = 0; r < (kTQ * kTK) / kAtThreads; ++r) {
            const auto [lq, lk] = at_tile_slot(tid, dir, r);
            const int qq = q0 + lq, k = k0 + lk;
            float z = at_neg_inf(), g = 0.0f;
            if (qq < nb && k < nb && (!v.mask || (v.mask[qq] && v.mask[k]))) {
                const size_t at = dir ? (size_t)k * N + qq : (size_t)qq * N + k;
                z = ((v.a[qq] + v.c[k]) + v.sc[at]) + v.kb;
                if (with_dw) g = dS[at];
            }
            s_z[lq][lk] = z;
            if (with_dw) s_g[lq][lk] = g;
        }
    };
    auto store_tile = [&](int k0) {  // s_z -> dS, inside the prefix (the whole matrix without sizes)
#pragma unroll
        for (int r = 0; r < (kTQ * kTK) / kAtThreads; ++r) {
            const auto [lq, lk] = at_tile_slot(tid, dir, r);
            const int qq = q0 + lq, k = k0 + lk;
            if (qq < nb && k < nb) dS[dir ? (size_t)k * N + qq : (size_t)qq * N + k] = s_z[lq][lk];
        }
    };

    // pass 1: dw[q,k] = dmsg[q] . val[k] into dS, and delta[q] = sum_k w dw.  That is dmsg[q] . msg[q], formed from
    // the numbers dz subtracts it from: the rounding of delta then cancels in sum_k dz as it does in exact
    // arithmetic, and one key gives exactly 0.
    float delta = 0.0f;
    for (int k0 = 0; k0 < nb; k0 += kTK) {
        load_z(k0, false);
        float dw[kTK / 16];
#pragma unroll
        for (int r = 0; r < kTK / 16; ++r) dw[r] = 0.0f;
        for (int d0 = 0; d0 < D; d0 += kDChunk) {
            const int dlen = (D - d0) < kDChunk ? (D - d0) : kDChunk;
            for (int idx = tid; idx < kTK * dlen; idx += kAtThreads) {
                const int k = idx / dlen, d = idx - k * dlen;
                s_v[k][d] = (k0 + k < nb) ? v.val[(size_t)(k0 + k) * hidden + d0 + d] : 0.0f;
            }
            for (int idx = tid; idx < kTQ * dlen; idx += kAtThreads) {
                const int lq = idx / dlen, d = idx - lq * dlen;
                s_dm[lq][d] = (q0 + lq < nb) ? v.dmsg[(size_t)(q0 + lq) * hidden + d0 + d] : 0.0f;
            }
            __syncthreads();
            for (int d = 0; d < dlen; ++d) {
                const float x = s_dm[cq][d];
#pragma unroll
                for (int r = 0; r < kTK / 16; ++r) dw[r] += x * s_v[slot + 16 * r][d];
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < kTK / 16; ++r) {
            const int k = slot + 16 * r;
            const float z = s_z[cq][k];
            if constexpr (DROP)
                dw[r] *= dual_dropout_factor(p.fwd.drop, kDropStreamAttn, drop_base + (size_t)q * N + (k0 + k));
            if (z != at_neg_inf()) {
                const float s = z >= 0.0f ? z : 0.2f * z;
                delta += (expf(s - mq) / sq) * dw[r];
            }
            s_z[cq][k] = dw[r];
        }
        __syncthreads();
        store_tile(k0);
        __syncthreads();
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) delta += __shfl_xor(delta, off, 16);

    // pass 2: dz from z, the statistics and the stored dw
    float da_acc = 0.0f;
    double dk_acc = 0.0;  // the workgroup's part of dkb: a sum that cancels, kept in fp64 from the first term
    for (int k0 = 0; k0 < nb; k0 += kTK) {
        load_z(k0, true);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kTK / 16; ++r) {
            const int k = slot + 16 * r;
            const float z = s_z[cq][k];
            float dz = 0.0f;
            if (z != at_neg_inf()) {
                const float s = z >= 0.0f ? z : 0.2f * z;
                const float w = expf(s - mq) / sq;
                dz = (w * (s_g[cq][k] - delta)) * (z >= 0.0f ? 1.0f : 0.2f);
            }
            s_z[cq][k] = dz;
            da_acc += dz;
            dk_acc += (double)dz;
        }
        __syncthreads();
        store_tile(k0);
        __syncthreads();
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        da_acc += __shfl_xor(da_acc, off, 16);
        dk_acc += __shfl_xor(dk_acc, off, 16);
    }
    if (slot == 0) {
        if (q < N) da[q] = da_acc;
        s_dk[cq] = dk_acc;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < kTQ; ++i) t += s_dk[i];
        *part = t;
    }
}

// Key-major: one workgroup per (16 keys, head, direction, instance) walks the query tiles, the forward with the
// roles swapped: dc[k] = sum_q dS[q,k] (read back) and dval[k] = sum_q w[q,k] dmsg[q] with w recomputed.
// DROP: dval[k] = sum_q w keep scale dmsg[q] with the element index of the query-major kernel.
template <bool DROP>
__global__ void __launch_bounds__(kAtThreads) dual_attention_bwd_key_kernel(DualAttnBwdParams p)
{
    __shared__ float s_w[kTQ][kTK + 1];   // [key][query]
    __shared__ float s_g[kTQ][kTK + 1];
    __shared__ float s_dm[kTK][kDChunk];
    const int tid = threadIdx.x;
    const int dir = blockIdx.z & 1, b = blockIdx.z >> 1, h = blockIdx.y;
    const int kk0 = blockIdx.x * kTQ;
    const int N = p.fwd.n, D = p.fwd.head_dim, heads = p.fwd.heads, hidden = heads * D;
    const AtBwdView v = at_bwd_view(p, b, dir, h);
    const int nb = v.nb;
    const float *dS = p.dS + (((size_t)b * 2 + dir) * heads + h) * (size_t)N * N;
    float *dc = (dir ? p.dc_col : p.dc_row) + v.bh * N;
    float *dval = (dir ? p.d_row_val : p.d_col_val) + v.node;
    const int ck = tid >> 4, slot = tid & 15;
    const unsigned long long drop_base = DROP ? at_drop_base(b, dir, h, heads, N) : 0;
    if (kk0 >= nb) {  // padded keys
        for (int idx = tid; idx < kTQ * D; idx += kAtThreads) {
            const int k = kk0 + idx / D;
            if (k < N) dval[(size_t)k * hidden + idx % D] = 0.0f;
        }
        if (tid < kTQ && kk0 + tid < N) dc[kk0 + tid] = 0.0f;
        return;
    }
    for (int d0 = 0; d0 < D; d0 += kDChunk) {
        const int dlen = (D - d0) < kDChunk ? (D - d0) : kDChunk;
        float acc[kDChunk / 16];
#pragma unroll
        for (int r = 0; r < kDChunk / 16; ++r) acc[r] = 0.0f;
        float dcs = 0.0f;
        for (int q0 = 0; q0 < nb; q0 += kTK) {
#pragma unroll
            for (int r = 0; r < (kTQ * kTK) / kAtThreads; ++r) {
                const auto [lk, lq] = at_tile_slot(tid, !dir, r);  // the roles swapped
                const int q = q0 + lq, k = kk0 + lk;
                float w = 0.0f, g = 0.0f;
                if (q < nb && k < nb && (!v.mask || (v.mask[q] && v.mask[k]))) {
                    const size_t at = dir ? (size_t)k * N + q : (size_t)q * N + k;
                    const float z = ((v.a[q] + v.c[k]) + v.sc[at]) + v.kb;
                    const float s = z >= 0.0f ? z : 0.2f * z;
                    w = expf(s - v.stats[(size_t)q * 2]) / v.stats[(size_t)q * 2 + 1];
                    if constexpr (DROP)
                        w *= dual_dropout_factor(p.fwd.drop, kDropStreamAttn, drop_base + (size_t)q * N + k);
                    g = dS[at];
                }
                s_w[lk][lq] = w;
                s_g[lk][lq] = g;
            }
            for (int idx = tid; idx < kTK * dlen; idx += kAtThreads) {
                const int lq = idx / dlen, d = idx - lq * dlen;
                s_dm[lq][d] = (q0 + lq < nb) ? v.dmsg[(size_t)(q0 + lq) * hidden + d0 + d] : 0.0f;
            }
            __syncthreads();
            for (int lq = 0; lq < kTK; ++lq) {
                const float w = s_w[ck][lq];
                dcs += s_g[ck][lq];
#pragma unroll
                for (int r = 0; r < kDChunk / 16; ++r) {
                    const int d = slot + 16 * r;
                    if (d < dlen) acc[r] += w * s_dm[lq][d];
                }
            }
            __syncthreads();
        }
        const int k = kk0 + ck;
        if (k < N) {
#pragma unroll
            for (int r = 0; r < kDChunk / 16; ++r) {
                const int d = slot + 16 * r;
                if (d < dlen) dval[(size_t)k * hidden + d0 + d] = acc[r];
            }
            if (d0 == 0 && slot == 0) dc[k] = dcs;
        }
    }
}

// dkb[dir][h]: the partials of the query-major workgroups, (instance, tile) in order, in fp64; one workgroup each
__global__ void __launch_bounds__(kAtThreads)
dual_attention_bwd_kbias_kernel(const double *partials, float *dkb, int batch, int heads, int tiles)
{
    __shared__ double s_sum[kAtThreads];
    const int dir = blockIdx.x / heads, h = blockIdx.x - dir * heads;
    const long long count = (long long)batch * tiles;
    double t = 0.0;
    for (long long i = threadIdx.x; i < count; i += kAtThreads) {
        const long long b = i / tiles, x = i - b * tiles;
        t += partials[((size_t)(2 * b + dir) * heads + h) * tiles + x];
    }
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int half = kAtThreads / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) dkb[blockIdx.x] = (float)s_sum[0];
}

// ---- the backward of the edge scores ---------------------------------------------------------------------------
// Stage 1 (dual_edge_backward_kernel) recomputes a wave tile of 16 edges in the forward's transposed layout and
// goes back through it: dh2 = G^T dS and dh1 = W2^T dh2pre are MFMA products whose A operand reads the staged G
// and W2 column-wise (Gs[(4 s + g) * stride + 16 m + col], W2s[(16 m + 4 g + r) * stride + 16 t + col]; the lane
// groups fall on disjoint banks) and whose B operand is already in registers.  The loop over m is the k loop of
// dh1, so it stays rolled with the eight accumulators of dh1 live.  Each edge leaves one row of kRowFloats floats in
// the workspace: h1, h2, dh2pre, dh1pre (128 each), dS (16, zero past 2 * heads) and the features (16: ten
// channels, a one in column 10, zeros); a lane without an edge leaves zeros where a product's A operand reads.
// Stage 2 (dual_edge_wgrad_kernel): out[o][k] = sum_e X[e][o] Y[e][k] on the same instruction, both fragments read
// along the contiguous unit index of the rows.  A workgroup owns a slice of the chunk's rows, wave w the tiles:
// dW2 row block w (8 tiles), dG column block w, dW1 row block w, and dh2pre^T F row block w, whose column 10 is
// db2 as column 10 of dW1's tile is db1.  Stage 3 sums the workgroups' partials in fp64 in order, adds the chunk
// to the running fp64 sums and, after the last chunk, rounds once.
// VGPRs / LDS / scratch: see the header of this file.

constexpr int kRowFloats = 4 * kHid + 2 * kOutPad;
constexpr int kRowH1 = 0, kRowH2 = kHid, kRowDh2 = 2 * kHid, kRowDh1 = 3 * kHid, kRowDs = 4 * kHid;
constexpr int kRowF = 4 * kHid + kOutPad;
constexpr int kOnesCol = kDualEdgeIn;          // the column of ones in the padded features
constexpr int kWgTiles = 88;                   // 64 of dW2, 8 of dG, 8 of dW1 | db1, 8 of db2
constexpr int kWgOut = kWgTiles * 256;
constexpr int kWgMaxBlocks = 128;
constexpr int kWgMinRows = 64;

__device__ __forceinline__ float gelu_grad(float x)
{
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
    return cdf + x * pdf;
}

// One wave tile, eb_wave_tile: two overloads picked by the staged weights' type, as es_wave_tile's.  f: the features of
// the lane's edge or null; ds: dS of the lane's edge (zeros for a lane without an edge and past 2 * heads); row: where
// the tile's rows go.  DROP: the recompute applies the forward's mask (`keep` from es_keep_bits), the row's h1 is the
// dropped one, which dW2 needs, and dx1 = dh1 * keep * scale * GELU'(x1).
//
// bf16 (the contract at the top of this file): the workspace holds, per wave tile, an image [544 units][16 edges] of
// bf16 in the unit order of the fp32 row (kRowH1 .. kRowF), so that a fragment of stage 2, eight consecutive edges of
// one unit, is one 16-byte load.  32 units at a time go through the wave's LDS buffer (eb_flush32): 2-byte LDS writes, one 16-byte
// read and one 16-byte global store per lane.  dh2 = G^T dS takes G^T and dh1 = W2^T dh2pre takes W2^T from their own
// staged images, so every A fragment is one LDS read; the loop walks two blocks of h2 at a time, one k-step of dh1.

// 32 units x 16 edges of a wave tile: v[4 half + r] is unit 16 half + 4 g + r of the lane's edge; dst is the image's
// first unit of the 32.  The LDS unit serves a wave's accesses in order; the fences keep the compiler from moving them.
__device__ __forceinline__ void eb_flush_copy(__bf16 *buf, __bf16 *dst, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bf16x8 out = *reinterpret_cast<const bf16x8 *>(buf + 8 * lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    *reinterpret_cast<bf16x8 *>(dst + 8 * lane) = out;
}

__device__ __forceinline__ void eb_flush32(__bf16 *buf, bf16x8 v, __bf16 *dst, int lane)
{
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) buf[(16 * (j >> 2) + 4 * g + (j & 3)) * kEsEdgesPerWave + col] = v[j];
    eb_flush_copy(buf, dst, lane);
}

// fp32: ds is dS of the lane's edge for the outputs 4 s + g, row the lane's workspace row.
template <bool DROP>
__device__ __forceinline__ void eb_wave_tile(const EsWeights &w, const float *f, const float (&ds)[4], float *row, int col,
                                             int g, unsigned keep = 0, float scale = 1.0f)
{
    float fb[3];
    es_feature_fragment(f, g, fb);
    f32x4 h1[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        h1[m] = es_first_layer<DROP>(w, fb, m, col, g, keep, scale);
        *reinterpret_cast<f32x4 *>(&row[kRowH1 + 16 * m + 4 * g]) = h1[m];
    }
    f32x4 dh1[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) dh1[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int m = 0; m < 8; ++m) {
        const f32x4 acc = es_second_layer(w, h1, m, col, g);
        *reinterpret_cast<f32x4 *>(&row[kRowH2 + 16 * m + 4 * g]) = gelu4(acc);
        f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(w.Gs[(4 * s + g) * kWStride + 16 * m + col], ds[s], d, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = d[r] * gelu_grad(acc[r]);
        *reinterpret_cast<f32x4 *>(&row[kRowDh2 + 16 * m + 4 * g]) = d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float *wr = &w.W2s[(16 * m + 4 * g + r) * kWStride + col];
#pragma unroll
            for (int t = 0; t < 8; ++t) dh1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * t], d[r], dh1[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {  // the first layer's pre-activation once more: three products, no register kept
        const f32x4 acc = es_first_pre(w, fb, t, col, g);
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = dh1[t][r] * gelu_grad(acc[r]);
        if constexpr (DROP) d = es_drop4(d, keep, t, scale);
        *reinterpret_cast<f32x4 *>(&row[kRowDh1 + 16 * t + 4 * g]) = d;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = 4 * s + g;
        row[kRowDs + k] = ds[s];
        row[kRowF + k] = s < 3 ? (k == kOnesCol ? (f ? 1.0f : 0.0f) : fb[s]) : 0.0f;
    }
}

// bf16: ds is dS of the lane's edge for the outputs 8 g + j (g < 2), row the wave tile's image.
template <bool DROP>
__device__ __forceinline__ void eb_wave_tile(const EsWeightsBf &w, const float *f, const float (&ds)[8], __bf16 *row,
                                             int col, int g, unsigned keep = 0, float scale = 1.0f)
{
    const int lane = 16 * g + col;
    const bf16x8 fb = bf_feature_fragment(f, g);
    bf16x8 dsb;
#pragma unroll
    for (int j = 0; j < 8; ++j) dsb[j] = (__bf16)ds[j];
    bf16x8 h1[4];
    bf_first_layer<DROP>(w, fb, col, g, keep, scale, h1);
#pragma unroll
    for (int s = 0; s < 4; ++s) eb_flush32(w.flush, h1[s], row + (kRowH1 + 32 * s) * kEsEdgesPerWave, lane);
    f32x4 dh1[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) dh1[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        f32x4 x2[2], d[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) x2[half] = bf_second_layer(w, h1, 2 * s + half, col, g);
        eb_flush32(w.flush, bf_pack(gelu4(x2[0]), gelu4(x2[1])), row + (kRowH2 + 32 * s) * kEsEdgesPerWave, lane);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int m = 2 * s + half;
            d[half] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf_k16_fragment(&w.GTs[(16 * m + col) * kBfK1], g), dsb,
                                                              f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) d[half][r] = d[half][r] * gelu_grad(x2[half][r]);
        }
        const bf16x8 dp = bf_pack(d[0], d[1]);
        eb_flush32(w.flush, dp, row + (kRowDh2 + 32 * s) * kEsEdgesPerWave, lane);
#pragma unroll
        for (int t = 0; t < 8; ++t)
            dh1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<const bf16x8 *>(&w.W2Ts[(16 * t + col) * kBfStride + 32 * s + 8 * g]), dp, dh1[t], 0, 0,
                0);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // the first layer's pre-activation once more
        f32x4 d[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int t = 2 * s + half;
            const f32x4 acc = es_first_pre(w, fb, t, col, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) d[half][r] = dh1[t][r] * gelu_grad(acc[r]);
            if constexpr (DROP) d[half] = es_drop4(d[half], keep, t, scale);
        }
        eb_flush32(w.flush, bf_pack(d[0], d[1]), row + (kRowDh1 + 32 * s) * kEsEdgesPerWave, lane);
    }
    // dS (16 units) and the features with their column of ones (16 units): the lane groups 0 and 1 hold them
    if (g < 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * g + j;
            w.flush[k * kEsEdgesPerWave + col] = dsb[j];
            w.flush[(kOutPad + k) * kEsEdgesPerWave + col] = k == kOnesCol ? (__bf16)(f ? 1.0f : 0.0f) : fb[j];
        }
    }
    eb_flush_copy(w.flush, row + kRowDs * kEsEdgesPerWave, lane);
}

// The wave tiles [t0, t1) of the batch: numbered 16 edges at a time in the linear edge order (sizes null) or as
// dual_edge_scores_ragged_kernel numbers them.  Wave tile t writes the rows 16 (t - t0) .. + 15 of `rows`: floats, or
// with BF16 the bf16 images of 16 edges (eb_wave_tile), half the bytes.
template <bool DROP, bool BF16>
__global__ void __launch_bounds__(kEsThreads)
dual_edge_backward_kernel(const float *F, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *G, const float *dS, const int *sizes, int batch, int N, int heads,
                          long long t0, long long t1, void *rows, DualDropout drop)
{
    const int outs = 2 * heads;
    const auto w = es_stage_weights<true>(std::bool_constant<BF16>{}, W1, b1, W2, b2, G, outs);
    typedef decltype(w) Staged;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const long long stride = (long long)gridDim.x * kEsWaves;
    const size_t NN = (size_t)N * N;
    long long next = t0 + (long long)blockIdx.x * kEsWaves + wave;
    // at: the edge's offset inside its instance's [n][n] plane, or -1
    auto tile = [&](long long t, int b, long long at) {
        float ds[Staged::kDsRegs];
#pragma unroll
        for (int s = 0; s < Staged::kDsRegs; ++s) {
            const int o = BF16 ? 8 * g + s : 4 * s + g;  // the k index of dS as the lane's fragment holds it
            ds[s] = (at >= 0 && o < outs) ? dS[((size_t)b * outs + o) * NN + (size_t)at] : 0.0f;
        }
        // the lane's row, or with BF16 the wave tile's image
        auto *row = static_cast<typename Staged::Row *>(rows) +
                    ((size_t)(t - t0) * kEsEdgesPerWave + (BF16 ? 0 : col)) * kRowFloats;
        // a lane without an edge has dS = 0, hence dx2 = dx1 = 0 whatever its bits are
        const unsigned keep = DROP ? es_keep_bits(drop, (unsigned long long)b * NN + (at >= 0 ? at : 0), g) : 0u;
        eb_wave_tile<DROP>(w, at >= 0 ? F + ((size_t)b * NN + (size_t)at) * kDualEdgeIn : nullptr, ds, row, col, g, keep,
                           drop.scale);
    };
    if (!sizes) {
        const long long E = (long long)NN * batch;
        for (; next < t1; next += stride) {
            const long long e = next * kEsEdgesPerWave + col;
            const long long b = e / (long long)NN;
            tile(next, (int)b, e < E ? e - b * (long long)NN : -1);
        }
        return;
    }
    long long first = 0;
    for (int b = 0; b < batch && first < t1; ++b) {
        const EsInstanceTiles it = es_instance_tiles(sizes[b], N);
        const long long end = first + it.count < t1 ? first + it.count : t1;
        for (; next < end; next += stride) {
            const int t = (int)(next - first);
            const int i = t / it.groups, j = (t - i * it.groups) * kEsEdgesPerWave + col;
            tile(next, b, j < it.n ? (long long)i * N + j : -1);
        }
        first += it.count;
    }
}

// rows of the chunk [t0, t1) that stage 1 wrote: all of them, or up to the last wave tile the sizes give
__device__ __forceinline__ long long eb_chunk_rows(const int *sizes, int batch, int N, long long t0, long long t1)
{
    if (sizes) {
        long long total = 0;
        for (int b = 0; b < batch; ++b) total += es_instance_tiles(sizes[b], N).count;
        t1 = total < t1 ? total : t1;
    }
    return t1 > t0 ? (t1 - t0) * kEsEdgesPerWave : 0;
}

// Stage 2, both precisions: a workgroup's slice [begin, end) of the chunk's rows (per and the chunk's row count are
// multiples of 16), the lane's place in its wave's tiles, and the eleven accumulators zeroed.
struct WgSlice {
    int wave, col, g;
    long long begin, end;
};

__device__ __forceinline__ WgSlice wg_begin(const int *sizes, int batch, int N, long long t0, long long t1, int per,
                                            f32x4 (&acc)[11])
{
    const long long nrows = eb_chunk_rows(sizes, batch, N, t0, t1);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long begin = (long long)blockIdx.x * per;
    const WgSlice s{wave, lane & 15, lane >> 4, begin, begin + per < nrows ? begin + per : nrows};
#pragma unroll
    for (int j = 0; j < 11; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    return s;
}

// the workgroup's partials: wave w owns the tiles 8 w + j of dW2 and the tile w of dG, dW1 | db1 and db2
__device__ __forceinline__ void wg_store(float *partials, const f32x4 (&acc)[11], const WgSlice &s)
{
    float *out = partials + (size_t)blockIdx.x * kWgOut;
#pragma unroll
    for (int j = 0; j < 11; ++j) {
        const int tile = j < 8 ? 8 * s.wave + j : 64 + 8 * (j - 8) + s.wave;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[tile * 256 + (4 * s.g + r) * 16 + s.col] = acc[j][r];
    }
}

__global__ void __launch_bounds__(kEsThreads)
dual_edge_wgrad_kernel(const float *rows, const int *sizes, int batch, int N, long long t0, long long t1, int per,
                       float *partials)
{
    f32x4 acc[11];
    const WgSlice s = wg_begin(sizes, batch, N, t0, t1, per, acc);
    const int wave = s.wave, col = s.col, g = s.g;
    for (long long e = s.begin; e < s.end; e += 4) {
        const float *row = rows + (size_t)(e + g) * kRowFloats;
        const float a2 = row[kRowDh2 + 16 * wave + col], a1 = row[kRowDh1 + 16 * wave + col];
        const float as = row[kRowDs + col], bf = row[kRowF + col], bh = row[kRowH2 + 16 * wave + col];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, row[kRowH1 + 16 * j + col], acc[j], 0, 0, 0);
        acc[8] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bh, acc[8], 0, 0, 0);
        acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bf, acc[9], 0, 0, 0);
        acc[10] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bf, acc[10], 0, 0, 0);
    }
    wg_store(partials, acc, s);
}

// The same five products on v_mfma_f32_16x16x32_bf16 from the bf16 images of stage 1: the edge is k, one k-step takes
// two wave tiles (lane groups 0, 1: edges 0..7, 8..15 of the first, groups 2, 3 of the second; a slice with an odd
// number of tiles ends with zero fragments there).  Every fragment is one 16-byte load; the partials keep their layout.
__global__ void __launch_bounds__(kEsThreads)
dual_edge_wgrad_bf16_kernel(const __bf16 *rows, const int *sizes, int batch, int N, long long t0, long long t1, int per,
                            float *partials)
{
    f32x4 acc[11];
    const WgSlice s = wg_begin(sizes, batch, N, t0, t1, per, acc);
    const int wave = s.wave, col = s.col, g = s.g;
    const long long tile_end = s.end / kEsEdgesPerWave;
    for (long long pair = s.begin / kEsEdgesPerWave; pair < tile_end; pair += 2) {  // wave-uniform
        const long long tile = pair + (g >> 1);
        const bool has = tile < tile_end;
        const __bf16 *image = rows + (size_t)(has ? tile : 0) * kEsEdgesPerWave * kRowFloats + 8 * (g & 1);
        auto frag = [&](int unit) {
            return has ? *reinterpret_cast<const bf16x8 *>(image + (size_t)unit * kEsEdgesPerWave) : bf_zero8();
        };
        const bf16x8 a2 = frag(kRowDh2 + 16 * wave + col), a1 = frag(kRowDh1 + 16 * wave + col);
        const bf16x8 as = frag(kRowDs + col), bf = frag(kRowF + col), bh = frag(kRowH2 + 16 * wave + col);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, frag(kRowH1 + 16 * j + col), acc[j], 0, 0, 0);
        acc[8] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as, bh, acc[8], 0, 0, 0);
        acc[9] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bf, acc[9], 0, 0, 0);
        acc[10] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bf, acc[10], 0, 0, 0);
    }
    wg_store(partials, acc, s);
}

// output idx of the partials = tile * 256 + row * 16 + column of the tile
__global__ void __launch_bounds__(256)
dual_edge_wgrad_reduce_kernel(const float *partials, int blocks, double *sums, int first, int last, float *dW1,
                              float *db1, float *dW2, float *db2, float *dG, int outs)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    double t = 0.0;
    for (int k = 0; k < blocks; ++k) t += (double)partials[(size_t)k * kWgOut + idx];
    if (!first) t += sums[idx];
    sums[idx] = t;
    if (!last) return;
    const float v = (float)t;
    const int tile = idx >> 8, r = (idx >> 4) & 15, c = idx & 15;
    if (tile < 64) {
        dW2[(16 * (tile >> 3) + r) * kHid + 16 * (tile & 7) + c] = v;
    } else if (tile < 72) {
        if (r < outs) dG[r * kHid + 16 * (tile - 64) + c] = v;
    } else if (tile < 80) {
        const int o = 16 * (tile - 72) + r;
        if (c < kDualEdgeIn) dW1[o * kDualEdgeIn + c] = v;
        if (c == kOnesCol) db1[o] = v;
    } else if (c == kOnesCol) {
        db2[16 * (tile - 80) + r] = v;
    }
}

constexpr size_t kEsLdsBytes = (size_t)kEsLdsFloats * sizeof(float);

// more dynamic LDS than the 64 KB default is allowed once per process and kernel, not on each of a forward's
// launches (and not inside a capture: the first launch is the uncaptured warm-up every captured call has).  The flag
// belongs to the kernel instantiation: one shared by two would leave the second without its attribute.
template <auto Kernel>
hipError_t es_raise_lds(size_t bytes)
{
    static std::atomic<bool> raised{false};
    if (!raised.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        raised.store(true, std::memory_order_release);
    }
    return hipSuccess;
}

// f(std::bool_constant...) of the runtime flags: where a launch picks its <DROP> or <DROP, BF16> instantiation
template <class F>
hipError_t dispatch_bools(bool a, F &&f)
{
    return a ? f(std::true_type{}) : f(std::false_type{});
}

template <class F>
hipError_t dispatch_bools(bool a, bool b, F &&f)
{
    return dispatch_bools(a, [&](auto A) { return dispatch_bools(b, [&](auto B) { return f(A, B); }); });
}

// the padded batch's wave tiles in the ragged numbering: the sizes are on the device, so grids and workspaces are
// sized for every instance at n
long long es_padded_tiles(int batch, int n) { return batch * es_instance_tiles(n, n).count; }

}  // namespace

size_t dual_gnn_workspace_bytes(int batch, int n, int heads)
{
    if (batch < 1 || batch > kDualMaxBatch || n < 1 || n > 16384 || heads < 1 || heads > kDualMaxHeads) return 0;
    const size_t bytes = (size_t)batch * 2 * heads * n * n * sizeof(float);
    return (bytes + 255) & ~(size_t)255;
}

namespace {

template <bool DROP, bool BF16>
hipError_t edge_scores(const DualEdgeParams &p, float *scores, hipStream_t stream)
{
    constexpr size_t lds = BF16 ? kEsBfFwdBytes : kEsLdsBytes;
    const long long NN = (long long)p.n * p.n, E = NN * p.batch;
    // a workgroup takes 8 wave tiles at a time; with sizes the grid is sized for the padded batch, and a workgroup
    // without a tile leaves
    const long long tiles = p.sizes ? (es_padded_tiles(p.batch, p.n) + kEsWaves - 1) / kEsWaves : (E + kEsTile - 1) / kEsTile;
    const dim3 grid((unsigned)(tiles < kEsMaxBlocks ? tiles : kEsMaxBlocks));
    if (p.sizes) {
        constexpr auto kernel = dual_edge_scores_ragged_kernel<DROP, BF16>;
        if (hipError_t e = es_raise_lds<kernel>(lds)) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(kEsThreads), lds, stream, p.edge_feat, p.W1, p.b1, p.W2, p.b2, p.G, scores,
                           p.sizes, p.batch, p.n, p.heads, p.drop);
    } else {
        constexpr auto kernel = dual_edge_scores_kernel<DROP, BF16>;
        if (hipError_t e = es_raise_lds<kernel>(lds)) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(kEsThreads), lds, stream, p.edge_feat, p.W1, p.b1, p.W2, p.b2, p.G, scores,
                           E, NN, p.heads, tiles, p.drop);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dual_edge_scores(const DualEdgeParams &p, float *scores, hipStream_t stream)
{
    return dispatch_bools(p.drop.on, p.bf16, [&](auto drop, auto bf16) {
        return edge_scores<decltype(drop)::value, decltype(bf16)::value>(p, scores, stream);
    });
}

hipError_t launch_dual_attention(const DualAttnParams &p, hipStream_t stream)
{
    const dim3 grid((p.n + kTQ - 1) / kTQ, p.heads, 2 * p.batch);
    return dispatch_bools(p.drop.on, [&](auto drop) {
        hipLaunchKernelGGL(dual_attention_kernel<decltype(drop)::value>, grid, dim3(kAtThreads), 0, stream, p);
        return hipGetLastError();
    });
}

__global__ void __launch_bounds__(256)
dual_dropout_keep_kernel(DualDropout drop, unsigned stream_id, unsigned long long first, unsigned long long count,
                         unsigned char *keep)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) keep[i] = dual_dropout_keep(drop, stream_id, first + i) ? 1 : 0;
}

hipError_t launch_dual_dropout_keep(const DualDropout &drop, unsigned stream_id, unsigned long long first,
                                    unsigned long long count, unsigned char *keep, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(dual_dropout_keep_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, drop,
                       stream_id, first, count, keep);
    return hipGetLastError();
}

namespace {

// The edge backward's workspace: the chunk's rows, the workgroups' partials, the running fp64 sums.  It depends on
// (batch, n) only through the padded batch's wave tiles, so the uniform and the ragged call share it.
struct EdgeBwdLayout {
    long long tiles;   // wave tiles of the padded batch in the ragged numbering (not fewer than the uniform one's)
    long long rows;    // rows of the largest chunk
    int per, blocks;   // rows per workgroup of stage 2 and its grid for a full chunk
    size_t partials_at, sums_at, bytes;
};

EdgeBwdLayout edge_bwd_layout(int batch, int n)
{
    EdgeBwdLayout l;
    l.tiles = es_padded_tiles(batch, n);
    const long long all = l.tiles * kEsEdgesPerWave;
    l.rows = all < kDualBwdChunk ? all : kDualBwdChunk;
    long long per = (l.rows + kWgMaxBlocks - 1) / kWgMaxBlocks;
    per = (per + 15) / 16 * 16;
    l.per = (int)(per < kWgMinRows ? kWgMinRows : per);
    l.blocks = (int)((l.rows + l.per - 1) / l.per);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    l.partials_at = up((size_t)l.rows * kRowFloats * sizeof(float));
    l.sums_at = l.partials_at + up((size_t)l.blocks * kWgOut * sizeof(float));
    l.bytes = l.sums_at + up((size_t)kWgOut * sizeof(double));
    return l;
}

}  // namespace

size_t dual_backward_workspace_bytes(int batch, int n, int heads)
{
    if (dual_gnn_workspace_bytes(batch, n, heads) == 0) return 0;
    const size_t attn = ((size_t)2 * batch * heads * ((n + kTQ - 1) / kTQ) * sizeof(double) + 255) & ~(size_t)255;
    const size_t edge = edge_bwd_layout(batch, n).bytes;
    return attn > edge ? attn : edge;
}

hipError_t launch_dual_attention_backward(const DualAttnBwdParams &p, hipStream_t stream)
{
    const DualAttnParams &f = p.fwd;
    const int tiles = (f.n + kTQ - 1) / kTQ;
    const dim3 grid(tiles, f.heads, 2 * f.batch);
    const hipError_t e = dispatch_bools(f.drop.on, [&](auto drop) {
        constexpr bool DROP = decltype(drop)::value;
        hipLaunchKernelGGL(dual_attention_bwd_query_kernel<DROP>, grid, dim3(kAtThreads), 0, stream, p);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(dual_attention_bwd_key_kernel<DROP>, grid, dim3(kAtThreads), 0, stream, p);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dual_attention_bwd_kbias_kernel, dim3(2 * f.heads), dim3(kAtThreads), 0, stream, p.partials,
                       p.dkb, f.batch, f.heads, tiles);
    return hipGetLastError();
}

namespace {

template <bool DROP, bool BF16>
hipError_t edge_scores_backward(const DualEdgeParams &p, const float *dS, const DualEdgeGrads &grads, void *workspace,
                                hipStream_t stream)
{
    const EdgeBwdLayout l = edge_bwd_layout(p.batch, p.n);
    const long long E = (long long)p.batch * p.n * p.n;
    const long long tiles = p.sizes ? l.tiles : (E + kEsEdgesPerWave - 1) / kEsEdgesPerWave;
    const long long chunk = kDualBwdChunk / kEsEdgesPerWave;
    // the chunk's rows first; BF16: bf16 images in the first half of the fp32 rows' room
    float *partials = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + l.partials_at);
    double *sums = reinterpret_cast<double *>(static_cast<unsigned char *>(workspace) + l.sums_at);
    constexpr size_t lds = BF16 ? kEsBfBwdBytes : kEsLdsBytes;
    constexpr auto kernel = dual_edge_backward_kernel<DROP, BF16>;
    if (hipError_t e = es_raise_lds<kernel>(lds)) return e;
    for (long long t0 = 0; t0 < tiles; t0 += chunk) {
        const long long t1 = t0 + chunk < tiles ? t0 + chunk : tiles;
        const long long wgs = (t1 - t0 + kEsWaves - 1) / kEsWaves;
        const int blocks = (int)(wgs < kEsMaxBlocks ? wgs : kEsMaxBlocks);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kEsThreads), lds, stream, p.edge_feat, p.W1, p.b1, p.W2, p.b2, p.G,
                           dS, p.sizes, p.batch, p.n, p.heads, t0, t1, workspace, p.drop);
        if (hipError_t e = hipGetLastError()) return e;
        const int wg = (int)(((t1 - t0) * kEsEdgesPerWave + l.per - 1) / l.per);
        if constexpr (BF16)
            hipLaunchKernelGGL(dual_edge_wgrad_bf16_kernel, dim3(wg), dim3(kEsThreads), 0, stream,
                               static_cast<const __bf16 *>(workspace), p.sizes, p.batch, p.n, t0, t1, l.per, partials);
        else
            hipLaunchKernelGGL(dual_edge_wgrad_kernel, dim3(wg), dim3(kEsThreads), 0, stream,
                               static_cast<const float *>(workspace), p.sizes, p.batch, p.n, t0, t1, l.per, partials);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(dual_edge_wgrad_reduce_kernel, dim3(kWgOut / 256), dim3(256), 0, stream, partials, wg, sums,
                           t0 == 0 ? 1 : 0, t1 == tiles ? 1 : 0, grads.dW1, grads.db1, grads.dW2, grads.db2, grads.dG,
                           2 * p.heads);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_dual_edge_scores_backward(const DualEdgeParams &p, const float *dS, const DualEdgeGrads &grads,
                                            void *workspace, hipStream_t stream)
{
    return dispatch_bools(p.drop.on, p.bf16, [&](auto drop, auto bf16) {
        return edge_scores_backward<decltype(drop)::value, decltype(bf16)::value>(p, dS, grads, workspace, stream);
    });
}

}  // namespace lapwarm
