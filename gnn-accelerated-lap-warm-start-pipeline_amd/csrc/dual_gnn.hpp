// dual_gnn.hpp -- the two kernels of DualGNN's fused DualLayer attention (dual_gnn.hip).
//
// edge scores:  scores[b][dir][h][i][j] = g_{dir,h} . GELU(W2 GELU(W1 f(i,j) + b1) + b2), both directions in the
//               natural [i][j] layout (nothing is stored transposed);
// attention:    both directions in one launch.  The column direction reads scores[b][1] through LDS tiles whose
//               global loads run along i's neighbour j, so its loads stay coalesced (16 queries x 64 keys per tile).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dual_dropout.hpp"

namespace lapwarm {

constexpr int kDualMaxHeads = 8;      // 2 * heads outputs fit the 16-wide MFMA tile
constexpr int kDualMaxBatch = 32767;  // the attention grid is (tiles, heads, 2 * batch)
constexpr int kDualEdgeHidden = 128;  // width of the edge MLP's two hidden layers (fixed by the model)
constexpr int kDualEdgeIn = 10;

struct DualAttnParams {
    const float *scores;              // [batch][2][heads][n][n]
    const float *a_row, *c_row;       // [batch][heads][n]: row direction, query i / key j
    const float *a_col, *c_col;       // [batch][heads][n]: column direction, query j / key i
    const float *kbias;               // [2][heads]
    const unsigned char *mask;        // [batch][n] (0: padded node) or null
    const float *row_val, *col_val;   // [batch][n][heads * head_dim]
    float *row_msg, *col_msg;         // [batch][n][heads * head_dim]
    int batch, n, heads, head_dim;
    // [batch] on the device, or null.  With sizes the mask is the prefix [0, sizes[b]) (a size outside 1..n: empty)
    // and `mask` is not read: a block of padded queries writes zeros and leaves, the key loops end with the last
    // tile that holds a key of the prefix, and no score outside the prefix is loaded.  The messages are, bit for bit,
    // those of the prefix mask: a masked key adds +0 to both sums.
    const int *sizes = nullptr;
    // [batch][heads][n][2] or null: the maximum and the sum of exp(s - max) of every query's softmax, for the
    // backward.  Null pointers leave the kernel's arithmetic and every message bit as they are.
    float *row_stats = nullptr, *col_stats = nullptr;
    // The dropout of the attention weights (stream 1 of dual_dropout.hpp), off by default: the weighted values use
    // w * keep * scale, the statistics stay those of the undropped softmax, and the backward regenerates the mask.
    DualDropout drop{};
};

// The backward of the attention (dual_gnn.hip): fwd holds the forward's inputs, its messages and its statistics
// (all read); partials is workspace of 2 * batch * heads * ceil(n / 16) doubles.
struct DualAttnBwdParams {
    DualAttnParams fwd;
    const float *d_row_msg, *d_col_msg;          // [batch][n][heads * head_dim]
    float *dS;                                   // [batch][2][heads][n][n], the scores' layout
    float *da_row, *dc_row, *da_col, *dc_col;    // [batch][heads][n]
    float *dkb;                                  // [2][heads]
    float *d_row_val, *d_col_val;                // [batch][n][heads * head_dim]
    double *partials;
};

// Edges per chunk of the edge-score backward: a chunk's workspace rows (544 floats per edge: h1, h2, dh2pre, dh1pre
// of 128 each, dS and the features padded to 16) take 30720 * 2176 B = 63.75 MiB.
constexpr int kDualBwdChunk = 30720;

// The edge MLP's call (dual_gnn.hip): scores[b][dir][h][i][j] from the features, both directions.
struct DualEdgeParams {
    const float *edge_feat;           // [batch][n][n][10]
    const float *W1, *b1, *W2, *b2;   // Linear(10, 128), Linear(128, 128)
    const float *G;                   // [2 * heads][128], the folded score weights
    // [batch] on the device, or null for the uniform batch.  A padded batch of instances of sizes[b] (a size outside
    // 1..n: no edge): only the edges (i, j < sizes[b]) are computed, a row's tail rounded up to 16 edges, and written;
    // scores outside the prefixes are left as they are.  On the prefixes the bits are the uniform batch's.
    const int *sizes;
    int batch, n, heads;
    // With drop.on, h1 = GELU(W1 f + b1) is replaced by keep * scale * h1 (stream 0 of dual_dropout.hpp) before the
    // second product.  drop.on false selects the kernels without the generator: their bits, whatever else drop holds.
    DualDropout drop{};
    // The edge MLP on the bf16 MFMA units (the contract in dual_gnn.hip).  The scores stay fp32; the mask of a seed is
    // the mask of the fp32 kernels.
    bool bf16 = false;
};

struct DualEdgeGrads {
    float *dW1, *db1, *dW2, *db2, *dG;  // the shapes of W1, b1, W2, b2, G
};

size_t dual_gnn_workspace_bytes(int batch, int n, int heads);  // the scores tensor; 0 for arguments out of range
hipError_t launch_dual_edge_scores(const DualEdgeParams &p, float *scores, hipStream_t stream);
// heads <= 65535 here (the grid's y dimension): kDualMaxHeads limits the edge-scores kernel and the workspace only
hipError_t launch_dual_attention(const DualAttnParams &p, hipStream_t stream);

// The workspace of either backward launch below (the larger of the two); 0 for arguments out of range.
size_t dual_backward_workspace_bytes(int batch, int n, int heads);
// Three kernels: query-major (dS, da, per-workgroup partials of dkb), key-major (dc, dval), the reduce of dkb.
hipError_t launch_dual_attention_backward(const DualAttnBwdParams &p, hipStream_t stream);
// Per chunk of kDualBwdChunk edges three kernels: the recompute (rows into the workspace), the TN products per
// workgroup slice, the fp64 reduce over workgroups and chunks.  dS: the gradient of the scores, in their layout.
// p.bf16: the backward of the bf16 forward, whose rows are bf16 and fit the same workspace.
hipError_t launch_dual_edge_scores_backward(const DualEdgeParams &p, const float *dS, const DualEdgeGrads &grads,
                                            void *workspace, hipStream_t stream);
// keep[i] = 1 if element first + i of the stream is kept, else 0, for i < count: the keep rule itself, for tests
hipError_t launch_dual_dropout_keep(const DualDropout &drop, unsigned stream_id, unsigned long long first,
                                    unsigned long long count, unsigned char *keep, hipStream_t stream);

}  // namespace lapwarm
