// dual_dropout.hpp -- the keep rule of the two dropouts inside DualGNN's fused region (dual_gnn.hip).
//
// A mask is never stored: whether element e of a logical tensor is kept is a pure function of (seed, stream, e), so
// the backward regenerates what the forward used, and tiling, chunking and `sizes` cannot change a mask.
//
//   Philox4x32-10 (philox.hpp): key (lo32(seed), hi32(seed)), counter (lo32(e >> 2), hi32(e >> 2), stream, 0);
//   the random word of e is output e & 3; e is kept iff word >= T, T = floor(p * 2^32) formed in double on the host;
//   a kept value is multiplied by float(1 / (1 - p)).
//
// Stream 0, the edge MLP after its first GELU: e = ((b N + i) N + j) 128 + unit.
// Stream 1, the attention weights:             e = (((b 2 + dir) H + h) N + q) N + k, q the query and k the key of
//                                              the direction (dir = 1: the query is the column j).
// Both index the PADDED layout.
#pragma once

#include <hip/hip_runtime.h>

#include "philox.hpp"

namespace lapwarm {

constexpr unsigned kDropStreamEdge = 0, kDropStreamAttn = 1;

struct DualDropout {
    unsigned k0 = 0, k1 = 0;    // the key: lo32(seed), hi32(seed)
    unsigned threshold = 0;     // T: keep iff word >= T
    float scale = 1.0f;         // float(1 / (1 - p))
    bool on = false;            // p > 0; off selects the kernels without the generator
};

// The four words of counter (lo32(group), hi32(group), stream, 0) under key (k0, k1); element e has group e >> 2.
__host__ __device__ __forceinline__ void dual_dropout_words(unsigned k0, unsigned k1, unsigned stream,
                                                            unsigned long long group, unsigned (&out)[4])
{
    philox4x32_10(k0, k1, stream, group, out);
}

// Element e alone (the attention kernels: one call per key that uses one word).
__host__ __device__ __forceinline__ bool dual_dropout_keep(const DualDropout &d, unsigned stream, unsigned long long e)
{
    unsigned w[4];
    dual_dropout_words(d.k0, d.k1, stream, e >> 2, w);
    const unsigned r = (unsigned)e & 3u;
    const unsigned word = r == 0 ? w[0] : r == 1 ? w[1] : r == 2 ? w[2] : w[3];
    return word >= d.threshold;
}

// The factor of element e: scale or 0.
__host__ __device__ __forceinline__ float dual_dropout_factor(const DualDropout &d, unsigned stream,
                                                              unsigned long long e)
{
    return dual_dropout_keep(d, stream, e) ? d.scale : 0.0f;
}

}  // namespace lapwarm
