// ragged_duals.hpp -- the dual utilities (row minima, feasibility projection, reduced costs) of a batch of cost
// matrices of different sizes (ragged_batch.hip).
#pragma once

#include "ragged_batch.hpp"

namespace lapwarm {

// The workspace of one call: a vector per instance that the column and row passes leave for the kernel that
// reduces it to gmin, the stop flag of every instance, and the word the host reads between chunks of rounds.
struct RaggedDualsWs {
    double *part;  // [batch][N]
    int *done;     // [batch]
    int *running;  // [1]
    size_t bytes;  // of the three, as the C ABI lays them out
};

// out[b][i] = min_{j < n_b} (C_b[i][j] - (v ? v[b][j] : 0)) for i < n_b and 0 for n_b <= i < N, NaN as np.min;
// ret[b] (may be null) 0, or 2 for an instance treated as empty.  One kernel.
hipError_t launch_rowmin_ragged(const RaggedBatch &g, const double *v, double *out, int *ret, hipStream_t stream);

// Before the first round: done[b] = 0 and ret[b] = 0; an instance treated as empty is done at once, with u, v
// all 0, gmin 0, ret 2.  rounds[b] = 0; u, v of every instance are set to 0 beyond its prefix.
hipError_t launch_project_init_ragged(const RaggedBatch &g, const RaggedDualsWs &w, double *u, double *v, double *gmin,
                                      int *rounds, int *ret, hipStream_t stream);

// One round of project_feasible for every instance that is not done: u_i = min(u_i, min_j (C_ij - v_j));
// cap_j = min_i (C_ij - u_i), v_j = min(v_j, cap_j); gmin = min_j (cap_j - v_j), which is min((C - u) - v);
// rounds[b] += 1; done[b] = gmin >= -tol.  *running is 1 afterwards if some instance is not done, else 0.
// Three kernels, two reads of C.
hipError_t launch_project_round_ragged(const RaggedBatch &g, const RaggedDualsWs &w, double *u, double *v, double tol,
                                       double *gmin, int *rounds, hipStream_t stream);

// gmin[b] = min((C_b - u) - v) (0 for an instance treated as empty), ret[b] (may be null) 0 or 2; with `out`
// (the layout of C) out = (C - u) - v on the prefix of every instance, minus gmin[b] where shift_nonneg and
// gmin[b] < 0.  Two kernels, three with `out`.
hipError_t launch_reduce_costs_ragged(const RaggedBatch &g, const RaggedDualsWs &w, const double *u, const double *v,
                                      int shift_nonneg, double *out, double *gmin, int *ret, hipStream_t stream);

}  // namespace lapwarm
