// dense_sweeps.hpp -- launchers of the dense sweep kernels (dense_sweeps.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lapwarm {

struct PreludeParams {
    const double *C;
    int n, batch;
    const double *u;  // [batch][n] duals the verify step uses (seed, or projected)
    const double *v;  // [batch][n]
    double eps, tight_eps;
    int rerun;        // 0: first pass; 1: only instances whose duals were projected
    double *u_tight;
    int *viol_cnt;    // [batch][n] candidates of the projection per row (first pass only)
    int *tight_cnt;
    uint32_t *tight_bits;
    int *inst_flags;
};
hipError_t launch_prelude(const PreludeParams &p, hipStream_t stream);
hipError_t launch_seed_prepare(const double *u_seed, const double *v_seed, double *u_work, double *v_work,
                               size_t count, int *flags, int n_flags, int *ring, int n_ring, hipStream_t stream);

// Gauss-Seidel projection of (u, v) for the instances flagged kFlagHasViolation; in place.
hipError_t launch_projection(const double *C, int n, int batch, double *u, double *v,
                             const int *viol_cnt, int *inst_flags, double eps, hipStream_t stream);

// The three stages in front of a ragged seeded solve (ragged_batch.hpp): every [batch][.] array has the padded
// stride N, and the tight-edge bitmap of instance b is n_b rows of ceil(n_b / 32) words at b * N * ceil(N / 32).
// The prepare step also leaves x, y = -1, ret = 2 and stats = 0 for the solver launches to overwrite.
struct RaggedBatch;
hipError_t launch_seed_prepare_ragged(const RaggedBatch &g, const double *u_seed, const double *v_seed, double *u_work,
                                      double *v_work, int *flags, long long *x, long long *y, int *ret,
                                      long long *stats, hipStream_t stream);
hipError_t launch_prelude_ragged(const PreludeParams &p, const RaggedBatch &g, hipStream_t stream);  // p.n = g.N
hipError_t launch_projection_ragged(const RaggedBatch &g, double *u, double *v, const int *viol_cnt, int *inst_flags,
                                    double eps, hipStream_t stream);

// out[b][j] = min_i (C[b][i][j] - (u ? u[b][i] : 0)); `partial` holds batch*chunks*n doubles.
int colmin_chunks(int n, int batch);
hipError_t launch_colmin(const double *C, int n, int batch, const double *u, double *out,
                         double *partial, hipStream_t stream);

// out[b][i] = min_j (C[b][i][j] - (v ? v[b][j] : 0))
hipError_t launch_rowmin(const double *C, int n, int batch, const double *v, double *out,
                         hipStream_t stream);

// R[b][i][j] = (C - u_i) - v_j - shift[b] ; gmin[b] = min_ij ((C - u_i) - v_j)
hipError_t launch_reduced_min(const double *C, int n, int batch, const double *u, const double *v,
                              double *gmin_partial, double *gmin, hipStream_t stream);
hipError_t launch_reduce_costs(const double *C, int n, int batch, const double *u, const double *v,
                               const double *gmin, int shift_nonneg, double *out, hipStream_t stream);
// one round of project_feasible's u/v caps: u = min(u, rowmin(C - v)) ; v = min(v, colmin(C - u))
hipError_t launch_cap_rows(const double *C, int n, int batch, double *u, const double *v,
                           hipStream_t stream);
hipError_t launch_cap_cols(const double *C, int n, int batch, const double *u, double *v,
                           double *partial, hipStream_t stream);

// 13 row statistics + 8 positional encodings (float32) and the 16 smallest costs per row.
struct FeatureParams {
    const double *C;
    int n, batch;
    const double *colmin;  // [batch][n]
    const float *posenc;   // [n][8] host-computed table
    float *feat;           // [batch][n][21]
    float *topk;           // [batch][n][16] ascending, +inf padded, or null
};
hipError_t launch_row_features(const FeatureParams &p, hipStream_t stream);

}  // namespace lapwarm
