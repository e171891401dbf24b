// philox.hpp -- the counter-based generator behind everything random that a kernel draws: DualGNN's dropout masks
// (dual_dropout.hpp) and the synthetic cost families (cost_families.hpp).
//
//   Philox4x32-10 (Salmon et al., SC'11): key (lo32(seed), hi32(seed)), counter (lo32(group), hi32(group), stream, 0).
//
// A value is a pure function of (seed, stream, element): nothing is stored and nothing is advanced, so tiling,
// chunking, layout and batch composition cannot change a bit.  How an element maps to a group and to the four words
// of that group is the business of the includer.
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

// The four words of counter (lo32(group), hi32(group), stream, 0) under key (k0, k1).
__host__ __device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned stream,
                                                       unsigned long long group, unsigned (&out)[4])
{
    unsigned c0 = (unsigned)group, c1 = (unsigned)(group >> 32), c2 = stream, c3 = 0u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

}  // namespace lapwarm
