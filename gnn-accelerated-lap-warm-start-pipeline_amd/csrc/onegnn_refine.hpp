// onegnn_refine.hpp -- OneGNN refinement aggregation (onegnn_refine.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

hipError_t launch_refine_aggregate(const float *topk16, const float *u_pre, const float *w1,
                                   const float *b1, float *out, float *wsum, int rows, int H,
                                   hipStream_t stream);

// Backward of the aggregation: grad_u [rows], grad_w1 / grad_b1 [H] from grad_out [rows][H] and grad_wsum [rows]
// (may be null).  `ws` holds refine_backward_workspace_bytes(rows, H) bytes; every word read is written first.
size_t refine_backward_workspace_bytes(int rows, int H);
hipError_t launch_refine_backward(const float *topk16, const float *u_pre, const float *w1, const float *b1,
                                  const float *grad_out, const float *grad_wsum, float *grad_u, float *grad_w1,
                                  float *grad_b1, int rows, int H, void *ws, hipStream_t stream);

}  // namespace lapwarm
