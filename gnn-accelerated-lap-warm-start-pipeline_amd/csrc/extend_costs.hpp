// extend_costs.hpp -- rectangular / cost-limited lapjv (extend_costs.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

// E [batch][n][n] = C [batch][n_rows][n_cols] in the top left corner, `fill` beside and below it,
// 0 in E[n_rows:, n_cols:] (LAP/_lapjv_cpp/_lapjv.pyx:84-95; fill = 0 without a cost limit)
hipError_t launch_extend_costs(const double *C, int batch, int n_rows, int n_cols, int n, double fill, double *E,
                               hipStream_t stream);
// _lapjv.pyx:115-122: xs, ys [batch][n] of the solve on E -> x [batch][n_rows], y [batch][n_cols] with -1
// for unmatched, matched [batch] and opt [batch] (either may be null); gath [batch][n_rows] scratch.
// Instances with ret != 0: x, y all -1, opt NaN, matched 0.
hipError_t launch_extended_finish(const double *C, int batch, int n_rows, int n_cols, int n, const int *xs,
                                  const int *ys, const int *ret, int *x, int *y, double *opt, int *matched,
                                  double *gath, hipStream_t stream);

}  // namespace lapwarm
