// train_loss.hpp -- launchers and workspace slots of the OneGNN and DualGNN training losses (train_loss.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

constexpr int kTrainLossMaxN = 16384;
constexpr int kTrainLossBadSize = 2;  // ret[b] of an instance whose size is outside 1..n
constexpr int kTlTerms = 4;           // terms[b]: dual_lower, feas, u_reg (DualGNN: v_reg), primal_upper

struct TrainLossParams {
    const float *C;           // [batch][n][n]
    int n, batch;
    int chunks;               // row chunks of the column pass
    int rows_per_wave;        // rows one wave of the hinge pass owns
    int hparts;               // hinge partial sums per instance (one per wave of the hinge grid)
    const int *sizes;         // [batch] n_b
    const float *u, *ut;      // [batch][n] u_pred, u_target
    float *v;                 // [batch][n] v_proj (0 on padded columns)
    int *arow;                // [batch][n] a_j, the row attaining v_j (-1 on padded columns)
    int *assign;              // [batch][n] greedy column of row i (-1 on padded rows)
    float *terms;             // [batch][kTlTerms]
    int *ret;                 // [batch]
    // workspace
    float *pval;              // [batch][chunks][n] partial column minima
    int *parg;                // [batch][chunks][n] their rows
    int *K;                   // [batch][n] K_j = #{i : h_ij > 0}
    int *R;                   // [batch][n] R_i = #{j : h_ij > 0}
    int *cnt;                 // [batch][n] cnt_i = #{j : a_j = i}
    int *ksum;                // [batch][n] sum of K_j over the columns with a_j = i
    unsigned *mkey;           // [batch][n] f32_key(min_j reduced_ij)
    int *mj;                  // [batch][n] the lowest column attaining it
    double *hpart;            // [batch][hparts] partial sums of h
    // the DualGNN loss only, behind everything the OneGNN entries lay out; vh == nullptr selects the OneGNN loss
    const float *vh;          // [batch][n] v_hint
    float *dj;                // [batch][n] d_j = vh_j - v_j
    double *vsum;             // [batch][n] S_i = sum of d_j over the columns with a_j = i, in ascending j
};

// fills chunks, rows_per_wave and hparts for this shape
void train_loss_plan(TrainLossParams *p);
// column pass, hinge pass, then one workgroup per instance: sums, row order, greedy, terms, ret; with p.vh the
// third term is v_reg and that workgroup also writes dj and vsum
hipError_t launch_train_loss_forward(const TrainLossParams &p, hipStream_t stream);
// grad_u[b][i] from the counts the forward left in the workspace; weights [3] on the device
hipError_t launch_train_loss_backward(const TrainLossParams &p, const float *weights, float grad_scale,
                                      float *grad_u, hipStream_t stream);
// DualGNN: grad_u[b][i] and grad_vh[b][j] from the counts, dj and vsum the forward left in the workspace
hipError_t launch_dual_loss_backward(const TrainLossParams &p, const float *weights, float grad_scale, float *grad_u,
                                     float *grad_vh, hipStream_t stream);

}  // namespace lapwarm
