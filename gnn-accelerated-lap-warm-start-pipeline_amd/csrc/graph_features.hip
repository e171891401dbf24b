// graph_features.hip -- the reference's compute_features (gnn/features.py:49-153) for a resident batch.
//
// Everything is computed in fp64 and rounded once to float32, as the row-feature kernel of dense_sweeps.hip does.
// The entropy is the reference's unstabilised exp(-C) form (not the row-feature kernel's), the tie share counts
// gap <= 1e-3, the rank denominator is n - 1 (ranks are 0 at n = 1), a MAD below 1e-9 becomes 1e-9.
// Every sum is an LDS tree over per-thread partial sums in a fixed order: equal inputs give equal bits.
#include "graph_features.hpp"

#include <atomic>

namespace lapwarm {
namespace {

constexpr int kGfThreads = 256;
constexpr int kTile = 32;
constexpr int kStats = 6;  // per row of a side: median, MAD, min, tie share, entropy, min(x - u) (column side)
constexpr double kGfEps = 1e-9;   // gnn/features.py:18
constexpr double kGfTau = 1e-3;   // gnn/features.py:17

size_t gf_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct GraphWs {
    double *Ct;    // [batch][n][n]
    double *stat;  // [2][batch][n][kStats]
    int *rank;     // [2][batch][n][n]: side 0 [i][j], side 1 [j][i]
    size_t bytes;
};

GraphWs graph_layout(void *ws, int batch, int n)
{
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    const size_t bnn = (size_t)batch * n * n;
    GraphWs w;
    size_t off = 0;
    w.Ct = reinterpret_cast<double *>(base + off);
    off += gf_align(bnn * sizeof(double));
    w.stat = reinterpret_cast<double *>(base + off);
    off += gf_align((size_t)2 * batch * n * kStats * sizeof(double));
    w.rank = reinterpret_cast<int *>(base + off);
    off += gf_align(2 * bnn * sizeof(int));
    w.bytes = off;
    return w;
}

__device__ __forceinline__ unsigned long long gf_order_key(double x)
{
    const long long bts = __double_as_longlong(x + 0.0);  // -0.0 -> +0.0
    return bts < 0 ? ~(unsigned long long)bts : ((unsigned long long)bts | 0x8000000000000000ull);
}

// One 32 x 32 tile of the transposed copy of one instance: C with row stride ldc, Ct with row stride S.
__device__ __forceinline__ void gf_transpose_tile(const double *C, size_t ldc, double *Ct, int n, int S)
{
    __shared__ double tile[kTile][kTile + 1];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i < n && j < n) tile[r][threadIdx.x] = C[(size_t)i * ldc + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < n && j < n) Ct[(size_t)j * S + i] = tile[threadIdx.x][r];
    }
}

__global__ void __launch_bounds__(kTile * 8) gf_transpose_kernel(const double *C, double *Ct, int n)
{
    const size_t base = (size_t)blockIdx.z * n * n;
    gf_transpose_tile(C + base, n, Ct + base, n, n);
}

// The ragged batch: tiles over the padded width, the copy of instance b at plane b of stride N.  A tile outside
// the prefix has nothing to copy (nothing reads the copy there).
__global__ void __launch_bounds__(kTile * 8) gf_transpose_ragged_kernel(RaggedBatch g, double *Ct)
{
    const int b = blockIdx.z, N = g.N;
    const int n = ragged_size(g, b);
    if ((int)blockIdx.y * kTile >= n || (int)blockIdx.x * kTile >= n) return;  // workgroup-uniform
    gf_transpose_tile(g.C + g.offsets[b], g.ld ? g.ld : n, Ct + (size_t)b * N * N, n, N);
}

// all threads get the result; `red` holds kGfThreads values
template <class Op>
__device__ __forceinline__ double gf_reduce(double v, double *red, Op op)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kGfThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

struct GfSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct GfMin { __device__ double operator()(double a, double b) const { return b < a ? b : a; } };
struct GfMax { __device__ double operator()(double a, double b) const { return b > a ? b : a; } };

// ascending bitonic sort of (key, idx) pairs, npad a power of two; ends with a barrier
__device__ __forceinline__ void gf_sort(unsigned long long *key, int *idx, int npad)
{
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (npad >> 1); t += kGfThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const bool up = (i & k) == 0;
                const unsigned long long ka = key[i], kb = key[p];
                const int ia = idx[i], ib = idx[p];
                const bool a_gt_b = ka > kb || (ka == kb && ia > ib);
                if (a_gt_b == up) {
                    key[i] = kb;
                    key[p] = ka;
                    idx[i] = ib;
                    idx[p] = ia;
                }
            }
            __syncthreads();
        }
    }
}

// One row of one side, by one workgroup: M its n values (a row of C, or of the transposed copy on the column
// side), u the instance's u or null, `out` its 14 node features, `st` its kStats statistics, `rk` its n ranks.
// npad: a power of two >= n.  The (key, index) order is total, so the sorted order does not depend on npad.
__device__ __forceinline__ void gf_row_body(const double *M, int n, int npad, const double *u, bool side,
                                            const float *posenc, float *out, double *st, int *rk)
{
    extern __shared__ __align__(16) unsigned char gf_lds[];
    double *x = reinterpret_cast<double *>(gf_lds);                        // [n] (npad reserved)
    unsigned long long *key = reinterpret_cast<unsigned long long *>(x + npad);  // [npad]
    double *red = reinterpret_cast<double *>(key + npad);                  // [kGfThreads]
    int *idx = reinterpret_cast<int *>(red + kGfThreads);                  // [npad]
    const int tid = threadIdx.x;
    for (int j = tid; j < npad; j += kGfThreads) {
        if (j < n) {
            const double v = M[j];
            x[j] = v;
            key[j] = gf_order_key(v);
        } else {
            key[j] = ~0ull;
        }
        idx[j] = j;
    }
    __syncthreads();
    double mn = __longlong_as_double(0x7ff0000000000000LL), mx = -mn, sum = 0.0, esum = 0.0, vm = mn;
    for (int j = tid; j < n; j += kGfThreads) {
        const double v = x[j];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        sum += v;
        esum += exp(-v);
        if (side && u) {
            const double d = v - u[j];
            vm = d < vm ? d : vm;
        }
    }
    mn = gf_reduce(mn, red, GfMin());
    mx = gf_reduce(mx, red, GfMax());
    sum = gf_reduce(sum, red, GfSum());
    esum = gf_reduce(esum, red, GfSum());
    if (side && u) vm = gf_reduce(vm, red, GfMin());
    const double mean = sum / (double)n;
    const double denom = esum + kGfEps;
    double var = 0.0, ent = 0.0;
    int ties = 0;
    for (int j = tid; j < n; j += kGfThreads) {
        const double v = x[j];
        const double d = v - mean;
        var += d * d;
        const double p = exp(-v) / denom;
        ent += p * log(p + kGfEps);
        ties += (v - mn <= kGfTau) ? 1 : 0;
    }
    var = gf_reduce(var, red, GfSum());
    ent = -gf_reduce(ent, red, GfSum());
    const double tie = gf_reduce((double)ties, red, GfSum()) / (double)n;
    const double sd = sqrt(var / (double)n);

    gf_sort(key, idx, npad);
    for (int p = tid; p < n; p += kGfThreads) rk[idx[p]] = p;
    const double med = (x[idx[(n - 1) >> 1]] + x[idx[n >> 1]]) * 0.5;
    __syncthreads();
    for (int j = tid; j < npad; j += kGfThreads) {
        key[j] = j < n ? gf_order_key(fabs(x[j] - med)) : ~0ull;
        idx[j] = j;
    }
    __syncthreads();
    gf_sort(key, idx, npad);
    double mad = (fabs(x[idx[(n - 1) >> 1]] - med) + fabs(x[idx[n >> 1]] - med)) * 0.5;
    if (mad < kGfEps) mad = kGfEps;

    if (tid == 0) {
        st[0] = med;
        st[1] = mad;
        st[2] = mn;
        st[3] = tie;
        st[4] = ent;
        st[5] = vm;
    }
    if (tid < kNodeFeatureDim) {
        double v;
        switch (tid) {
        case 0: v = mn; break;
        case 1: v = mx; break;
        case 2: v = mean; break;
        case 3: v = sd; break;
        case 4: v = mad; break;
        case 5: v = ent; break;
        default: v = 0.0; break;
        }
        out[tid] = tid < 6 ? (float)v : posenc[tid - 6];
    }
}

// One workgroup per row of one side.  blockIdx.y = 2 * b + side; side 0 reads C, side 1 the transposed copy.
__global__ void __launch_bounds__(kGfThreads)
gf_row_kernel(const double *C, const double *Ct, const double *u, const float *posenc, float *row_out, float *col_out,
              double *stat, int *rank, int n, int npad, int batch)
{
    const int row = blockIdx.x, b = blockIdx.y >> 1, side = blockIdx.y & 1;
    const size_t at = ((size_t)side * batch + b) * n + row;
    gf_row_body((side ? Ct : C) + ((size_t)b * n + row) * n, n, npad, u ? u + (size_t)b * n : nullptr, side,
                posenc + (size_t)row * 8, (side ? col_out : row_out) + ((size_t)b * n + row) * kNodeFeatureDim,
                stat + at * kStats, rank + at * n);
}

// The ragged batch: grid (N, 2 * batch), every plane with the padded stride N.  A workgroup beyond its instance's
// prefix writes its zero row and is gone before the first barrier; npad is the instance's own power of two.
__global__ void __launch_bounds__(kGfThreads)
gf_row_ragged_kernel(RaggedBatch g, GraphFeatureRaggedOut o, const double *Ct, double *stat, int *rank)
{
    const int row = blockIdx.x, b = blockIdx.y >> 1, side = blockIdx.y & 1, N = g.N;
    const int n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
    float *out = (side ? o.col_out : o.row_out) + ((size_t)b * N + row) * kNodeFeatureDim;
    if (side == 0 && threadIdx.x == 0) {
        o.mask[(size_t)b * N + row] = row < n ? 1 : 0;
        if (row == 0) o.ret[b] = n ? 0 : 2;
    }
    if (row >= n) {  // workgroup-uniform
        if (threadIdx.x < kNodeFeatureDim) out[threadIdx.x] = 0.0f;
        return;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;
    const double *M = side ? Ct + ((size_t)b * N + row) * N : g.C + g.offsets[b] + (size_t)row * (g.ld ? g.ld : n);
    const size_t at = ((size_t)side * g.batch + b) * N + row;
    gf_row_body(M, n, npad, o.u ? o.u + (size_t)b * N : nullptr, side, o.posenc + ((size_t)o.pos_off[b] + row) * 8, out,
                stat + at * kStats, rank + at * N);
}

// One 32 x 32 tile of the edges of instance b by one workgroup: the column-side ranks, stored [j][i], are transposed
// through LDS.  C has row stride ldc; every other plane (ranks, statistics, u, edge) has stride S >= n, and the
// edges of the tile outside the n x n prefix, which exist when S > n, are written as zeros.
__device__ __forceinline__ void gf_edge_tile(const double *C, size_t ldc, const double *u, const double *stat,
                                             const int *rank, float *edge, int n, int S, int b, int batch)
{
    __shared__ int tile[kTile][kTile + 1];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const size_t bnn = (size_t)b * S * S;
    const int *rank0 = rank + bnn;
    const int *rank1 = rank + ((size_t)batch * S * S + bnn);
    const double *st0 = stat + (size_t)b * S * kStats;
    const double *st1 = stat + ((size_t)batch + b) * S * kStats;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < n && j < n) tile[r][threadIdx.x] = rank1[(size_t)j * S + i];
    }
    __syncthreads();
    const double rden = n > 1 ? (double)(n - 1) : 1.0;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i >= S || j >= S) continue;
        float f[kEdgeFeatureDim];
        if (i < n && j < n) {
            const double c = C[(size_t)i * ldc + j];
            const double *ri = st0 + (size_t)i * kStats, *cj = st1 + (size_t)j * kStats;
            f[0] = (float)((c - ri[0]) / ri[1]);
            f[1] = (float)((double)rank0[(size_t)i * S + j] / rden);
            f[2] = (float)((double)tile[threadIdx.x][r] / rden);
            f[3] = (float)(c - ri[2]);
            f[4] = (float)(c - cj[2]);
            f[5] = (float)ri[3];
            f[6] = (float)cj[3];
            f[7] = (float)ri[4];
            f[8] = (float)cj[4];
            f[9] = u ? (float)((c - u[(size_t)b * S + i]) - cj[5]) : 0.0f;
        } else {
#pragma unroll
            for (int k = 0; k < kEdgeFeatureDim; ++k) f[k] = 0.0f;
        }
        float2 *o = reinterpret_cast<float2 *>(edge + (bnn + (size_t)i * S + j) * kEdgeFeatureDim);
#pragma unroll
        for (int k = 0; k < kEdgeFeatureDim / 2; ++k) o[k] = make_float2(f[2 * k], f[2 * k + 1]);
    }
}

__global__ void __launch_bounds__(kTile * 8)
gf_edge_kernel(const double *C, const double *u, const double *stat, const int *rank, float *edge, int n, int batch)
{
    const int b = blockIdx.z;
    gf_edge_tile(C + (size_t)b * n * n, n, u, stat, rank, edge, n, n, b, batch);
}

// The ragged batch: all N x N tiles of every instance, zeros outside its prefix.
__global__ void __launch_bounds__(kTile * 8)
gf_edge_ragged_kernel(RaggedBatch g, const double *u, const double *stat, const int *rank, float *edge)
{
    const int b = blockIdx.z;
    const int n = ragged_size(g, b);
    gf_edge_tile(g.C + (n ? g.offsets[b] : 0), g.ld ? g.ld : n, u, stat, rank, edge, n, g.N, b, g.batch);
}

int gf_npad(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

constexpr size_t gf_row_lds(int npad) { return (size_t)npad * (8 + 8 + 4) + kGfThreads * 8; }

// More dynamic LDS than the 64 KB default, allowed once per process and kernel, and always the limit of the
// largest n, never this call's size: later calls with another n then need no further host call (and none inside
// a capture).
hipError_t gf_raise_lds(const void *kernel, std::atomic<bool> &raised)
{
    if (!raised.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)gf_row_lds(kGraphMaxN));
        if (e != hipSuccess) return e;
        raised.store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

size_t graph_features_workspace_bytes(int batch, int n)
{
    if (batch < 1 || batch > kGraphMaxBatch || n < 1 || n > kGraphMaxN) return 0;
    return graph_layout(nullptr, batch, n).bytes;
}

size_t graph_features_ragged_workspace_bytes(int batch, int N) { return graph_features_workspace_bytes(batch, N); }

hipError_t launch_graph_features(const GraphFeatureParams &p, void *ws, hipStream_t stream)
{
    const GraphWs w = graph_layout(ws, p.batch, p.n);
    const int n = p.n, npad = gf_npad(n);
    const int tiles = (n + kTile - 1) / kTile;
    const dim3 tgrid(tiles, tiles, p.batch), tblock(kTile, 8);
    hipLaunchKernelGGL(gf_transpose_kernel, tgrid, tblock, 0, stream, p.C, w.Ct, n);
    static std::atomic<bool> raised{false};
    if (hipError_t e = gf_raise_lds(reinterpret_cast<const void *>(gf_row_kernel), raised)) return e;
    hipLaunchKernelGGL(gf_row_kernel, dim3(n, 2 * p.batch), dim3(kGfThreads), gf_row_lds(npad), stream, p.C, w.Ct, p.u,
                       p.posenc, p.row_out, p.col_out, w.stat, w.rank, n, npad, p.batch);
    hipLaunchKernelGGL(gf_edge_kernel, tgrid, tblock, 0, stream, p.C, p.u, w.stat, w.rank, p.edge, n, p.batch);
    return hipGetLastError();
}

hipError_t launch_graph_features_ragged(const RaggedBatch &g, const GraphFeatureRaggedOut &o, void *ws,
                                        hipStream_t stream)
{
    if (g.batch < 1 || g.batch > kGraphMaxBatch || g.N < 1 || g.N > kGraphMaxN) return hipErrorInvalidValue;
    const GraphWs w = graph_layout(ws, g.batch, g.N);
    const int tiles = (g.N + kTile - 1) / kTile;
    const dim3 tgrid(tiles, tiles, g.batch), tblock(kTile, 8);
    hipLaunchKernelGGL(gf_transpose_ragged_kernel, tgrid, tblock, 0, stream, g, w.Ct);
    static std::atomic<bool> raised{false};
    if (hipError_t e = gf_raise_lds(reinterpret_cast<const void *>(gf_row_ragged_kernel), raised)) return e;
    // (the LDS of the largest instance the batch may hold; a workgroup lays out its own npad inside it)
    hipLaunchKernelGGL(gf_row_ragged_kernel, dim3(g.N, 2 * g.batch), dim3(kGfThreads), gf_row_lds(gf_npad(g.N)), stream,
                       g, o, w.Ct, w.stat, w.rank);
    hipLaunchKernelGGL(gf_edge_ragged_kernel, tgrid, tblock, 0, stream, g, o.u, w.stat, w.rank, o.edge);
    return hipGetLastError();
}

}  // namespace lapwarm
