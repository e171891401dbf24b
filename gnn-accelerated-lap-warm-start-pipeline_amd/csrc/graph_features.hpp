// graph_features.hpp -- DualGNN's edge, row and column features of a resident batch (graph_features.hip).
//
// Three kernels on the caller's stream: a tiled transpose of C, ONE row kernel that runs over C (row side) and
// over the transposed copy (column side), and an assembly kernel that writes the (B, n, n, 10) edge records.
// Ranks are stable (among equal values the lower index ranks first).  For every n the row kernel sorts
// (order key, index) pairs of the row in LDS with a bitonic network: the sorted position of an element is its
// rank and the two middle elements are the median, so no separate selection is needed; the median absolute
// deviation is a second sort of |x - median|.  Sorting at every n is a choice, not a measured optimum:
// rank-by-counting over the row in LDS (O(n^2) compares per row, but no barrier steps) may well be cheaper at
// small n than the log^2 n barrier steps of the network.  It is not used because the median and the MAD need the
// sorted order anyway, so counting would be a second code path next to the sort, not in place of it; the two
// have not been timed against each other.  The row (8 B), its keys (8 B) and indices (4 B) live in LDS:
// n <= kGraphMaxN.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ragged_batch.hpp"

namespace lapwarm {

constexpr int kGraphMaxN = 4096;
constexpr int kGraphMaxBatch = 32767;  // the row kernel's grid is (n, 2 * batch)
constexpr int kEdgeFeatureDim = 10;
constexpr int kNodeFeatureDim = 14;

struct GraphFeatureParams {
    const double *C;     // [batch][n][n]
    const double *u;     // [batch][n] or null: channel 9 is then 0
    const float *posenc; // [n][8]
    int batch, n;
    float *edge;         // [batch][n][n][10]
    float *row_out;      // [batch][n][14]
    float *col_out;      // [batch][n][14]
};

// 0 for batch or n outside 1..kGraphMaxBatch / 1..kGraphMaxN
size_t graph_features_workspace_bytes(int batch, int n);
hipError_t launch_graph_features(const GraphFeatureParams &p, void *ws, hipStream_t stream);

// The same features for a batch of instances of different sizes (ragged_batch.hpp), padded to N, in the same three
// kernels: each is the uniform kernel's body per instance, so the prefix of instance b -- edge[b][:n_b][:n_b],
// row_out[b][:n_b], col_out[b][:n_b] -- holds, bit for bit, what launch_graph_features gives instance b alone, and
// everything outside it is 0, as the reference's collate pads.  Every element of every output is written.
struct GraphFeatureRaggedOut {
    const double *u;       // [batch][N], read on each prefix, or null: channel 9 is then 0
    const float *posenc;   // [rows][8]: the per-n tables of the distinct sizes, one after the other
    const int *pos_off;    // [batch]: first table row of instance b
    float *edge;           // [batch][N][N][10]
    float *row_out;        // [batch][N][14]
    float *col_out;        // [batch][N][14]
    unsigned char *mask;   // [batch][N] 1 on the prefix
    int *ret;              // [batch] 0, or 2 for an instance treated as empty (all-zero outputs)
};

// the workspace with the padded stride N; 0 for batch or N outside 1..kGraphMaxBatch / 1..kGraphMaxN
size_t graph_features_ragged_workspace_bytes(int batch, int N);
hipError_t launch_graph_features_ragged(const RaggedBatch &g, const GraphFeatureRaggedOut &o, void *ws,
                                        hipStream_t stream);

}  // namespace lapwarm
