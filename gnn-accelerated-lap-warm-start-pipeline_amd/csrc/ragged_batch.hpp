// ragged_batch.hpp -- a batch of square fp64 cost matrices of different sizes, and the two sweeps that
// turn it into what one OneGNN step consumes (ragged_batch.hip; the row-feature kernel is an instantiation
// of the row body in dense_sweeps.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lapwarm {

// The limits of every dense entry point: a row of n values is what the row kernels keep in LDS, and the batch
// (or the heads) is the y dimension of a grid.
constexpr int kMaxN = 16384;
constexpr int kMaxGridY = 65535;

// The (batch, N) of a ragged call: 0, or the C ABI's argument code (-2 empty or too many instances, -5 N too large).
inline int check_ragged_dims(int batch, int N)
{
    if (N <= 0 || batch <= 0 || batch > kMaxGridY) return -2;
    if (N > kMaxN) return -5;
    return 0;
}

// Instance b is the n_b x n_b matrix at C + offsets[b] with row stride ld, or n_b when ld == 0 (packed).
// offsets are multiples of 8 bytes only.  N is the padded width of every output.
struct RaggedBatch {
    const double *C;
    const long long *offsets;  // [batch], elements, device
    const int *sizes;          // [batch], device
    int ld, batch, N;
};

// n_b, or 0 for an instance that is treated as empty: a size outside 1..N, or wider than its row stride
__device__ __forceinline__ int ragged_size(const RaggedBatch &g, int b)
{
    const int n = g.sizes[b];
    return (n >= 1 && n <= g.N && (g.ld == 0 || n <= g.ld)) ? n : 0;
}

// out[b][j] = min_{i < n_b} (C_b[i][j] - (u ? u[b][i] : 0)) for j < n_b and 0 for n_b <= j < N, NaN as np.min;
// u, out [batch][N].  One kernel.
hipError_t launch_colmin_ragged(const RaggedBatch &g, const double *u, double *out, hipStream_t stream);

// gmin[b] = min_{i, j < n_b} ((C_b[i][j] - u[b][i]) - v[b][j]), NaN as np.min, 0 for an instance treated as
// empty: launch_reduced_min per instance.  u, v, rowpart [batch][N]; gmin [batch].  Two kernels, the first two of
// launch_reduce_costs_ragged (ragged_duals.hpp).
hipError_t launch_reduced_min_ragged(const RaggedBatch &g, const double *u, const double *v, double *rowpart,
                                     double *gmin, hipStream_t stream);

struct RaggedFeatureOut {
    const double *colmin;  // [batch][N] from launch_colmin_ragged(g, nullptr, ...)
    const float *posenc;   // [rows][8]: the per-n tables of the distinct sizes, one after the other
    const int *pos_off;    // [batch]: first table row of instance b
    float *feat;           // [batch][N][21], 0 on padded rows
    float *topk;           // [batch][N][16] ascending, +inf beyond n_b and on padded rows, or null
    float *cost32;         // [batch][N][N] (float)C on the prefix, 0 elsewhere, or null
    unsigned char *mask;   // [batch][N] 1 on the prefix, or null
    int *ret;              // [batch] 0, or 2 for an instance treated as empty
};
hipError_t launch_row_features_ragged(const RaggedBatch &g, const RaggedFeatureOut &o, hipStream_t stream);

}  // namespace lapwarm
