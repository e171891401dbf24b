// onegnn_refine.hpp -- OneGNN refinement aggregation (onegnn_refine.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

hipError_t launch_refine_aggregate(const float *topk16, const float *u_pre, const float *w1,
                                   const float *b1, float *out, float *wsum, int rows, int H,
                                   hipStream_t stream);

}  // namespace lapwarm
