// cost_families.hpp -- the synthetic cost families, drawn on the device straight into a ragged batch
// (cost_families.hip): the draw rules, the families and the launches.
//
// Every value is a pure function of (seed, stream, element), with Philox4x32-10 as philox.hpp keys and counts it;
// `seed` is one 64-bit value per instance and `e` the element index inside the instance's logical tensor (e = i n + j
// in the n x n matrix).
//
//   dbl(hi, lo) = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, in [0, 1).
//   U_s(e): group e >> 1, dbl(w[2 (e & 1)], w[2 (e & 1) + 1]).
//   Z_s(e): group e >> 1, u1 = dbl(w0, w1), u2 = dbl(w2, w3), r = sqrt(-2 log(1 - u1)), t = 6.283185307179586 u2,
//           r cos(t) for even e and r sin(t) for odd e; fp64, every operation rounded, no FMA of the caller's.
//   I_s(e, m) = (w[e & 3] of group e >> 2) m >> 32, in [0, m).
//
// Streams: 0 element uniforms (U0), 1 element normals (Z1), 2 factor a, 3 factor b, 4 mask uniforms and tie integers,
// 5 repair integers.
//
// Families (parameters p0, p1 of the instance; every operation rounded, in the order written):
//   0 uniform       C = U0(e)
//   1 metric        p[k][d] = 100 U0(2 k + d); C = sqrt(dx dx + dy dy), dx = p[i][0] - p[j][0], dy likewise
//   2 low_rank      rank p0, sigma p1: a_ik = Z2(i rank + k), b_jk = Z3(j rank + k); S = 0 + a_i0 b_j0 + a_i1 b_j1 ...
//                   in ascending k; C = max(S + sigma Z1(e), 0)
//   3 clustered     blocks p0, noise p1: size = max(1, n / max(1, blocks)), blk(i) = min(i / size, blocks - 1);
//                   C = max((U0(e) - (blk(i) == blk(j) ? 0.4 : 0)) + noise Z1(e), 0)
//   4 noisy_linear  rank p0, noise p1: T = S + noise Z1(e); C = T - min_e T
//   5 tie           bins p0, jitter p1: m = max(1, bins); C = double(I4(e, m)) / double(m) + jitter U0(e)
//   6 sparse        sparsity p1: keep(e) = U4(e) < sparsity; a row i without a kept entry keeps (i, I5(i, n)); after
//                   that a column j without a kept entry keeps (I5(n + j, n), j); C = keep ? U0(e) : 1e6
// max(x, 0) is x > 0 ? x : 0.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "philox.hpp"
#include "ragged_batch.hpp"

namespace lapwarm {

enum CostFamily {
    kFamUniform = 0,
    kFamMetric = 1,
    kFamLowRank = 2,
    kFamClustered = 3,
    kFamNoisyLinear = 4,
    kFamTie = 5,
    kFamSparse = 6,
    kFamCount = 7,
};

constexpr unsigned kStreamU0 = 0, kStreamZ1 = 1, kStreamFactorA = 2, kStreamFactorB = 3, kStreamMask = 4,
                   kStreamRepair = 5;
constexpr int kMaxRank = 64;
constexpr int kCostTileRows = 8;     // rows of one workgroup: two for each of its four waves
constexpr int kCostTileCols = 128;   // elements of one pass of a wave over its row: a Philox group per lane

struct PhiloxKey {
    unsigned k0, k1;
};
__host__ __device__ __forceinline__ PhiloxKey philox_key(unsigned long long seed)
{
    return PhiloxKey{(unsigned)seed, (unsigned)(seed >> 32)};
}

__host__ __device__ __forceinline__ double draw_dbl(unsigned hi, unsigned lo)
{
    const unsigned long long bits = ((unsigned long long)(hi >> 5) << 26) | (unsigned long long)(lo >> 6);
    return (double)bits * 0x1p-53;
}

// U_s(2 g) and U_s(2 g + 1)
__host__ __device__ __forceinline__ void uniform_pair(PhiloxKey key, unsigned stream, unsigned long long g, double &x0,
                                                      double &x1)
{
    unsigned w[4];
    philox4x32_10(key.k0, key.k1, stream, g, w);
    x0 = draw_dbl(w[0], w[1]);
    x1 = draw_dbl(w[2], w[3]);
}
__host__ __device__ __forceinline__ double uniform_at(PhiloxKey key, unsigned stream, unsigned long long e)
{
    double x0, x1;
    uniform_pair(key, stream, e >> 1, x0, x1);
    return (e & 1) ? x1 : x0;
}

// Z_s(2 g) and Z_s(2 g + 1): the one place the normals are made, whichever of the two a caller wants
// (not inlined: the constants of log and sincos would otherwise stay in scalar registers across a caller's row loop)
__device__ __noinline__ inline double2 normal_pair_of(unsigned k0, unsigned k1, unsigned stream, unsigned long long g)
{
    unsigned w[4];
    philox4x32_10(k0, k1, stream, g, w);
    const double u1 = draw_dbl(w[0], w[1]), u2 = draw_dbl(w[2], w[3]);
    const double r = sqrt(-2.0 * log(1.0 - u1));
    const double t = 6.283185307179586 * u2;
    double s, c;
    sincos(t, &s, &c);
    return make_double2(r * c, r * s);
}
__device__ __forceinline__ void normal_pair(PhiloxKey key, unsigned stream, unsigned long long g, double &z0, double &z1)
{
    const double2 z = normal_pair_of(key.k0, key.k1, stream, g);
    z0 = z.x;
    z1 = z.y;
}

__host__ __device__ __forceinline__ int integer_of_word(unsigned word, int m)
{
    return (int)(((unsigned long long)word * (unsigned long long)(unsigned)m) >> 32);
}
// I_s(e, m), m >= 1
__host__ __device__ __forceinline__ int integer_at(PhiloxKey key, unsigned stream, unsigned long long e, int m)
{
    unsigned w[4];
    philox4x32_10(key.k0, key.k1, stream, e >> 2, w);
    const unsigned r = (unsigned)e & 3u;
    return integer_of_word(r == 0 ? w[0] : r == 1 ? w[1] : r == 2 ? w[2] : w[3], m);
}

// The workspace of one call.  Instance b owns fa[b N 64 ...] (a_ik at i rank + k; the metric points at 2 k + d),
// fb[b 64 N ...] (b_jk at k N + j), part[b tiles ...] (the minimum of T over each row tile), colany[b N ...] (1 where
// a column of the sparse family keeps an entry).
struct CostFamiliesWs {
    double *fa, *fb, *part;
    unsigned char *colany;
    size_t bytes;  // as the C ABI lays them out
};
__host__ __device__ inline int cost_tiles(int N) { return (N + kCostTileRows - 1) / kCostTileRows; }

struct CostFamiliesArgs {
    double *C;                          // the layout of a RaggedBatch: offsets, sizes, ld (0: packed), batch, N
    const long long *offsets;
    const int *sizes;
    int ld, batch, N;
    const int *family;                  // [batch]
    const unsigned long long *seeds;    // [batch]
    const double *params;               // [batch][4]: (rank | blocks | bins, sigma | noise | jitter | sparsity, 0, 0)
    int *ret;                           // [batch]: 0, 2 (size outside 1..N or wider than ld), 3 (family or rank)
    CostFamiliesWs ws;
};

// Three kernels, each one grid over all instances: the factors, points and flags of the workspace; the elements,
// over (row tile, instance); the minimum of noisy_linear and the column repairs of sparse.  Nothing outside the
// prefix of an instance is written.
hipError_t launch_generate_costs_ragged(const CostFamiliesArgs &a, hipStream_t stream);

// out[i] = U (kind 0, fp64), Z (kind 1, fp64) or I(., m) (kind 2, int32) of element first + i of `stream_id`, by the
// device functions the kernels use.
hipError_t launch_cost_family_draws(unsigned long long seed, unsigned stream_id, int kind, unsigned long long first,
                                    unsigned long long count, int m, void *out, hipStream_t stream);

}  // namespace lapwarm
