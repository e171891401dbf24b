// cost_families.hip -- the synthetic cost families of the reference's dataset generator (data/generators.py,
// SYNTHETIC_FAMILIES, restated from their definitions in cost_families.hpp) written straight into a ragged batch on
// the device, gfx950.  Three kernels, each one grid over all instances:
//
//   prepare   what an element needs from outside its own Philox groups: the factors a and b (low_rank,
//             noisy_linear), the points (metric), cleared column flags (sparse); ret[b].
//   elements  grid (row tile, instance).  A wave owns a row at a time and a lane one Philox group at a time: the two
//             neighbouring elements 2 g and 2 g + 1 of the instance's logical tensor, made together and stored together
//             where they lie in one row and on a 16-byte boundary (a packed instance starts on an 8-byte boundary and
//             a row of odd length on either, so the first and the last group of a row may hold one element of it).
//             noisy_linear leaves T and the tile's minimum, sparse its row repairs and the columns that keep an entry.
//   finish    noisy_linear: C = T - min T, the minimum reduced from the tiles'.  sparse: the column repairs.
//
// Deterministic: no floating-point atomics and no atomics at all.  The minimum goes through the reduction template
// of device_utils.hpp; a row's "keeps an entry" is a wave reduction; a column's is a flag that every writer sets to 1.
#include "cost_families.hpp"
#include "device_utils.hpp"

namespace lapwarm {

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerTile = kThreads / kWave;
static_assert(kCostTileCols == 2 * kWave, "one pass of a wave over its row: a group of two elements per lane");
static_assert(kCostTileRows % kWavesPerTile == 0, "every wave of a tile owns as many rows");
constexpr double kSparseFill = 1000000.0;  // data/generators.py:68

struct OrI32 {
    using T = int;
    static __device__ __forceinline__ T identity() { return 0; }
    static __device__ __forceinline__ T combine(T o, T v) { return v | o; }
};

// What the kernels know of instance b: n = 0 and family < 0 for one that gets no work.
struct Instance {
    int n, family, ret;
    int q;       // rank, blocks or bins
    double s;    // sigma, noise, jitter or sparsity
    PhiloxKey key;
};

__device__ __forceinline__ int param_int(double p)
{
    return !(p >= 0.0) ? 0 : (p >= 2147483647.0 ? 2147483647 : (int)p);
}

__device__ __forceinline__ Instance instance_of(const CostFamiliesArgs &a, int b)
{
    Instance t;
    const int n = a.sizes[b];
    t.n = (n >= 1 && n <= a.N && (a.ld == 0 || n <= a.ld)) ? n : 0;
    t.family = a.family[b];
    t.q = param_int(a.params[4 * (size_t)b]);
    t.s = a.params[4 * (size_t)b + 1];
    t.key = philox_key(a.seeds[b]);
    t.ret = 0;
    const bool factors = t.family == kFamLowRank || t.family == kFamNoisyLinear;
    if (t.n == 0)
        t.ret = 2;
    else if (t.family < 0 || t.family >= kFamCount || (factors && (t.q < 1 || t.q > kMaxRank)))
        t.ret = 3;
    if (t.ret) {
        t.n = 0;
        t.family = -1;
    }
    return t;
}

__global__ void __launch_bounds__(kThreads) cost_prepare_kernel(CostFamiliesArgs a)
{
    const int b = blockIdx.y, N = a.N;
    const Instance t = instance_of(a, b);
    const unsigned tid = blockIdx.x * kThreads + threadIdx.x, step = gridDim.x * kThreads;
    if (tid == 0) a.ret[b] = t.ret;
    const unsigned n = t.n;
    if (t.family == kFamLowRank || t.family == kFamNoisyLinear) {
        const unsigned rank = t.q, count = n * rank;  // <= 2^20
        double *fa = a.ws.fa + (size_t)b * N * kMaxRank, *fb = a.ws.fb + (size_t)b * N * kMaxRank;
        for (unsigned g = tid; 2 * g < count; g += step) {
            double z0, z1;
            normal_pair(t.key, kStreamFactorA, g, z0, z1);
            fa[2 * g] = z0;
            if (2 * g + 1 < count) fa[2 * g + 1] = z1;
            normal_pair(t.key, kStreamFactorB, g, z0, z1);
            const unsigned j0 = (2 * g) / rank, k0 = 2 * g - j0 * rank;
            fb[(size_t)k0 * N + j0] = z0;
            if (2 * g + 1 < count) {
                const unsigned j1 = (k0 + 1 == rank) ? j0 + 1 : j0, k1 = (k0 + 1 == rank) ? 0 : k0 + 1;
                fb[(size_t)k1 * N + j1] = z1;
            }
        }
    } else if (t.family == kFamMetric) {
        double *pts = a.ws.fa + (size_t)b * N * kMaxRank;
        for (unsigned k = tid; k < n; k += step) {
            double x, y;
            uniform_pair(t.key, kStreamU0, k, x, y);
            pts[2 * k] = 100.0 * x;
            pts[2 * k + 1] = 100.0 * y;
        }
    } else if (t.family == kFamSparse) {
        for (unsigned j = tid; j < n; j += step) a.ws.colany[(size_t)b * N + j] = 0;
    }
}

// What a wave needs of its row to make an element of it.
struct RowCtx {
    int i, n, N;
    const double *fa_i;  // a_i. (low_rank, noisy_linear) or the point of row i (metric)
    const double *fb;    // b (k N + j) or the points (2 j + d)
    int rank;
    double s;
    int size, blocks, blk_i;  // clustered
};

__device__ __forceinline__ double factor_sum(const RowCtx &r, int j)
{
    double S = 0.0;
    for (int k = 0; k < r.rank; ++k) S = S + r.fa_i[k] * r.fb[(size_t)k * r.N + j];
    return S;
}

// One row of one instance by one wave; `lane` owns the groups g_first + lane, + 64, ...  Returns what the family
// reduces over the row: the minimum of T (noisy_linear) or whether an entry is kept (sparse), per lane.
template <int FAM>
__device__ __forceinline__ void row_elements(const Instance &t, const RowCtx &r, double *row, int lane,
                                             unsigned char *colflag, double &tmin, int &kept)
{
    const unsigned n = r.n, e_row = (unsigned)r.i * n, e_end = e_row + n;
    const unsigned g_last = (e_end - 1) >> 1;
    for (unsigned g = (e_row >> 1) + lane; g <= g_last; g += kWave) {
        const unsigned e0 = 2 * g;
        const bool in0 = e0 >= e_row, in1 = e0 + 1 < e_end;
        const int j0 = (int)(e0 - e_row), j1 = j0 + 1;  // j0 = -1 where the group starts in the row above
        double x0 = 0.0, x1 = 0.0;
        if constexpr (FAM == kFamUniform) {
            uniform_pair(t.key, kStreamU0, g, x0, x1);
        } else if constexpr (FAM == kFamMetric) {
            const double px = r.fa_i[0], py = r.fa_i[1];
            if (in0) {
                const double dx = px - r.fb[2 * j0], dy = py - r.fb[2 * j0 + 1];
                x0 = sqrt(dx * dx + dy * dy);
            }
            if (in1) {
                const double dx = px - r.fb[2 * j1], dy = py - r.fb[2 * j1 + 1];
                x1 = sqrt(dx * dx + dy * dy);
            }
        } else if constexpr (FAM == kFamLowRank || FAM == kFamNoisyLinear) {
            double z0, z1;
            normal_pair(t.key, kStreamZ1, g, z0, z1);
            if (in0) x0 = factor_sum(r, j0) + r.s * z0;
            if (in1) x1 = factor_sum(r, j1) + r.s * z1;
            if constexpr (FAM == kFamLowRank) {
                x0 = x0 > 0.0 ? x0 : 0.0;
                x1 = x1 > 0.0 ? x1 : 0.0;
            } else {
                if (in0) tmin = __builtin_fmin(tmin, x0);
                if (in1) tmin = __builtin_fmin(tmin, x1);
            }
        } else if constexpr (FAM == kFamClustered) {
            double u0, u1, z0, z1;
            uniform_pair(t.key, kStreamU0, g, u0, u1);
            normal_pair(t.key, kStreamZ1, g, z0, z1);
            const int jj0 = in0 ? j0 : 0, jj1 = in1 ? j1 : 0;
            const int b0 = min(jj0 / r.size, r.blocks - 1), b1 = min(jj1 / r.size, r.blocks - 1);
            x0 = (u0 - (b0 == r.blk_i ? 0.4 : 0.0)) + r.s * z0;
            x1 = (u1 - (b1 == r.blk_i ? 0.4 : 0.0)) + r.s * z1;
            x0 = x0 > 0.0 ? x0 : 0.0;
            x1 = x1 > 0.0 ? x1 : 0.0;
        } else if constexpr (FAM == kFamTie) {
            double u0, u1;
            uniform_pair(t.key, kStreamU0, g, u0, u1);
            unsigned w[4];
            philox4x32_10(t.key.k0, t.key.k1, kStreamMask, g >> 1, w);  // elements 2 g, 2 g + 1 of group (2 g) >> 2
            const unsigned w0 = (g & 1) ? w[2] : w[0], w1 = (g & 1) ? w[3] : w[1];
            const double m = (double)r.blocks;
            x0 = (double)integer_of_word(w0, r.blocks) / m + r.s * u0;
            x1 = (double)integer_of_word(w1, r.blocks) / m + r.s * u1;
        } else {
            double u0, u1, m0, m1;
            uniform_pair(t.key, kStreamU0, g, u0, u1);
            uniform_pair(t.key, kStreamMask, g, m0, m1);
            const bool k0 = in0 && m0 < r.s, k1 = in1 && m1 < r.s;
            x0 = k0 ? u0 : kSparseFill;
            x1 = k1 ? u1 : kSparseFill;
            if (k0) colflag[j0] = 1;  // (every writer writes 1)
            if (k1) colflag[j1] = 1;
            kept |= (k0 || k1) ? 1 : 0;
        }
        double *p = row + j0;
        if (in0 && in1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<double2 *>(p) = make_double2(x0, x1);
        } else {
            if (in0) p[0] = x0;
            if (in1) p[1] = x1;
        }
    }
}

template <int FAM>
__device__ __forceinline__ void tile_elements(const CostFamiliesArgs &a, const Instance &t, int b, int i0,
                                              BlockExchange *ex, unsigned char *colflag)
{
    const int n = t.n, N = a.N;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const size_t stride = a.ld ? a.ld : n;
    double *base = a.C + a.offsets[b];
    const double *fa = a.ws.fa + (size_t)b * N * kMaxRank, *fb = a.ws.fb + (size_t)b * N * kMaxRank;
    if constexpr (FAM == kFamSparse) {
        for (int j = threadIdx.x; j < n; j += kThreads) colflag[j] = 0;
        __syncthreads();
    }
    RowCtx r;
    r.n = n;
    r.N = N;
    r.s = t.s;
    r.rank = t.q;
    r.fb = (FAM == kFamMetric) ? fa : fb;
    r.blocks = t.q;
    r.size = 1;
    if constexpr (FAM == kFamClustered) {
        const int d = t.q > 1 ? t.q : 1, size = n / d;
        r.size = size > 1 ? size : 1;
    }
    if constexpr (FAM == kFamTie) r.blocks = t.q > 1 ? t.q : 1;  // m
    double tmin = pos_inf();
    for (int i = i0 + wave; i < i0 + kCostTileRows && i < n; i += kWavesPerTile) {
        r.i = i;
        r.fa_i = (FAM == kFamMetric) ? fa + 2 * (size_t)i : fa + (size_t)i * r.rank;
        r.blk_i = min(i / r.size, r.blocks - 1);
        int kept = 0;
        double *row = base + (size_t)i * stride;
        row_elements<FAM>(t, r, row, lane, colflag, tmin, kept);
        if constexpr (FAM == kFamSparse) {
            if (!wave_reduce<OrI32>(kept)) {  // the row repair: (i, I5(i, n)) is kept
                const int jr = integer_at(t.key, kStreamRepair, (unsigned long long)i, n);
                drain();  // the fill that another lane stored there has landed
                if (lane == 0) {
                    row[jr] = uniform_at(t.key, kStreamU0, (unsigned long long)i * n + jr);
                    colflag[jr] = 1;
                }
            }
        }
    }
    if constexpr (FAM == kFamNoisyLinear) {
        BlockCtx bc;
        bc.init(ex);
        tmin = bc.min_f64<FminF64>(tmin);
        if (threadIdx.x == 0) a.ws.part[(size_t)b * cost_tiles(N) + i0 / kCostTileRows] = tmin;
    }
    if constexpr (FAM == kFamSparse) {
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += kThreads)
            if (colflag[j]) a.ws.colany[(size_t)b * N + j] = 1;  // (every writer writes 1)
    }
}

__global__ void __launch_bounds__(kThreads) cost_elements_kernel(CostFamiliesArgs a)
{
    __shared__ BlockExchange ex;
    __shared__ unsigned char colflag[kMaxN];
    const int b = blockIdx.y, i0 = blockIdx.x * kCostTileRows;
    const Instance t = instance_of(a, b);
    if (i0 >= t.n) return;  // a tile below the prefix, or an instance without work: workgroup-uniform
    switch (__builtin_amdgcn_readfirstlane(t.family)) {
    case kFamUniform: tile_elements<kFamUniform>(a, t, b, i0, &ex, colflag); break;
    case kFamMetric: tile_elements<kFamMetric>(a, t, b, i0, &ex, colflag); break;
    case kFamLowRank: tile_elements<kFamLowRank>(a, t, b, i0, &ex, colflag); break;
    case kFamClustered: tile_elements<kFamClustered>(a, t, b, i0, &ex, colflag); break;
    case kFamNoisyLinear: tile_elements<kFamNoisyLinear>(a, t, b, i0, &ex, colflag); break;
    case kFamTie: tile_elements<kFamTie>(a, t, b, i0, &ex, colflag); break;
    default: tile_elements<kFamSparse>(a, t, b, i0, &ex, colflag); break;
    }
}

// The same tiles again.  noisy_linear: every tile reduces the tiles' minima to the instance's (the same value in
// every tile: one order) and subtracts it from its rows.  sparse: thread j of the first ceil(n / 256) tiles looks
// after column j.
__global__ void __launch_bounds__(kThreads) cost_finish_kernel(CostFamiliesArgs a)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.y, N = a.N;
    const Instance t = instance_of(a, b);
    const int n = t.n;
    if (t.family == kFamNoisyLinear) {
        const int i0 = blockIdx.x * kCostTileRows;
        if (i0 >= n) return;
        const int tiles = (n + kCostTileRows - 1) / kCostTileRows;
        const double *part = a.ws.part + (size_t)b * cost_tiles(N);
        double m = pos_inf();
        for (int k = threadIdx.x; k < tiles; k += kThreads) m = __builtin_fmin(m, part[k]);
        BlockCtx bc;
        bc.init(&ex);
        m = bc.min_f64<FminF64>(m);
        const size_t stride = a.ld ? a.ld : n;
        double *base = a.C + a.offsets[b];
        for (int i = i0; i < i0 + kCostTileRows && i < n; ++i) {
            double *row = base + (size_t)i * stride;
            for (int j = threadIdx.x; j < n; j += kThreads) row[j] = row[j] - m;
        }
    } else if (t.family == kFamSparse) {
        const int j = blockIdx.x * kThreads + threadIdx.x;
        if (j < n && !a.ws.colany[(size_t)b * N + j]) {
            const int ir = integer_at(t.key, kStreamRepair, (unsigned long long)n + j, n);
            const size_t stride = a.ld ? a.ld : n;
            a.C[a.offsets[b] + (size_t)ir * stride + j] = uniform_at(t.key, kStreamU0, (unsigned long long)ir * n + j);
        }
    }
}

__global__ void __launch_bounds__(kThreads)
cost_family_draws_kernel(PhiloxKey key, unsigned stream_id, int kind, unsigned long long first,
                         unsigned long long count, int m, void *out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const unsigned long long e = first + i;
    if (kind == 0) {
        reinterpret_cast<double *>(out)[i] = uniform_at(key, stream_id, e);
    } else if (kind == 1) {
        double z0, z1;
        normal_pair(key, stream_id, e >> 1, z0, z1);
        reinterpret_cast<double *>(out)[i] = (e & 1) ? z1 : z0;
    } else {
        reinterpret_cast<int *>(out)[i] = integer_at(key, stream_id, e, m);
    }
}

}  // namespace

hipError_t launch_generate_costs_ragged(const CostFamiliesArgs &a, hipStream_t stream)
{
    if (check_ragged_dims(a.batch, a.N)) return hipErrorInvalidValue;
    const dim3 block(kThreads), tiles(cost_tiles(a.N), a.batch);
    hipLaunchKernelGGL(cost_prepare_kernel, dim3((a.N + 31) / 32, a.batch), block, 0, stream, a);
    hipLaunchKernelGGL(cost_elements_kernel, tiles, block, 0, stream, a);
    hipLaunchKernelGGL(cost_finish_kernel, tiles, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cost_family_draws(unsigned long long seed, unsigned stream_id, int kind, unsigned long long first,
                                    unsigned long long count, int m, void *out, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(cost_family_draws_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       stream, philox_key(seed), stream_id, kind, first, count, m, out);
    return hipGetLastError();
}

}  // namespace lapwarm
