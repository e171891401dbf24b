// extend_ragged.hpp -- cold lapjv of a batch of different sizes and shapes (extend_ragged.hip): what surrounds the
// ragged launches of jv_instance_kernel in lapwarm_lapjv_ragged and lapwarm_lapjv_extended_ragged.
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

// x, y [batch][N] = -1, ret [batch] = 2, stats [batch][32] = 0 (stats may be null): what an instance keeps when
// no solver launch of a square ragged cold solve takes it.
hipError_t launch_lapjv_ragged_init(long long *x, long long *y, int *ret, long long *stats, int batch, int N,
                                    hipStream_t stream);

// Instance b is the n_rows[b] x n_cols[b] matrix at C + offsets[b], rows ld apart (0: n_cols[b], packed), with its
// own cost_limit (+inf: none).  Its extended size n_b is lapwarm_lapjv_extended_n's; E_b [n_b][n_b] is packed at
// E + e_off[b].  An instance is treated as empty (e_n[b] = 0: no E, no solve, x and y -1, opt NaN, ret 2) when its
// shape on the device is not one the host planned for: n_rows outside 1..R, n_cols outside 1..Q or above ld > 0,
// non-square without extend_cost, n_b > N, or E_b would end beyond e_total.
struct ExtRagged {
    const double *C;
    const long long *offsets;  // [batch] elements, device
    const int *n_rows, *n_cols;  // [batch] device
    const double *limits;      // [batch] device
    int ld, extend_cost, batch;
    int R, Q, N;               // widths of x, of y, and the largest extended size (the solver's stride)
    long long e_total;         // elements of the E area
    long long *e_off;          // [batch] workspace, written by launch_extend_shapes
    int *e_n;                  // [batch] workspace, written by launch_extend_shapes
    double *E;                 // 16-byte aligned
};

// e_n and e_off (the exclusive scan of n_b^2) from the device shapes: one workgroup.
hipError_t launch_extend_shapes(const ExtRagged &g, hipStream_t stream);
// All E_b in one launch (_lapjv.pyx:84-95 per instance: C in the top left corner, cost_limit / 2. beside and below
// it, 0 in E[n_rows:, n_cols:]; 0 everywhere around C without a limit).  A square instance without a limit is
// copied like the rest: one extra pass over a small matrix buys one code path and one solver launch chain.
// Also sets ret [batch] = 2 and stats [batch][32] = 0 (stats may be null) ahead of the solver launches.
hipError_t launch_extend_costs_ragged(const ExtRagged &g, int *ret, long long *stats, hipStream_t stream);
// _lapjv.pyx:115-122 per instance: xs, ys [batch][N] int64 of the solves on E -> x [batch][R], y [batch][Q] int32
// with -1 for unmatched and for padding, matched [batch], opt [batch] (either may be null); gath [batch][R] scratch.
// Instances with ret != 0: x, y all -1, opt NaN, matched 0.
hipError_t launch_extended_finish_ragged(const ExtRagged &g, const long long *xs, const long long *ys, const int *ret,
                                         int *x, int *y, double *opt, int *matched, double *gath, hipStream_t stream);

}  // namespace lapwarm
