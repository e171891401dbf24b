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

__global__ void __launch_bounds__(kTile * 8) gf_transpose_kernel(const double *C, double *Ct, int n)
{
    __shared__ double tile[kTile][kTile + 1];
    const size_t base = (size_t)blockIdx.z * n * n;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i < n && j < n) tile[r][threadIdx.x] = C[base + (size_t)i * n + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < n && j < n) Ct[base + (size_t)j * n + i] = tile[threadIdx.x][r];
    }
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

// One workgroup per row of one side.  blockIdx.y = 2 * b + side; side 0 reads C, side 1 the transposed copy.
__global__ void __launch_bounds__(kGfThreads)
gf_row_kernel(const double *C, const double *Ct, const double *u, const float *posenc, float *row_out, float *col_out,
              double *stat, int *rank, int n, int npad, int batch)
{
    extern __shared__ __align__(16) unsigned char gf_lds[];
    double *x = reinterpret_cast<double *>(gf_lds);                        // [n] (npad reserved)
    unsigned long long *key = reinterpret_cast<unsigned long long *>(x + npad);  // [npad]
    double *red = reinterpret_cast<double *>(key + npad);                  // [kGfThreads]
    int *idx = reinterpret_cast<int *>(red + kGfThreads);                  // [npad]
    const int tid = threadIdx.x;
    const int row = blockIdx.x, b = blockIdx.y >> 1, side = blockIdx.y & 1;
    const double *M = (side ? Ct : C) + ((size_t)b * n + row) * n;
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
            const double d = v - u[(size_t)b * n + j];
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
    int *rk = rank + (((size_t)side * batch + b) * n + row) * n;
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
        double *st = stat + (((size_t)side * batch + b) * n + row) * kStats;
        st[0] = med;
        st[1] = mad;
        st[2] = mn;
        st[3] = tie;
        st[4] = ent;
        st[5] = vm;
    }
    float *out = (side ? col_out : row_out) + ((size_t)b * n + row) * kNodeFeatureDim;
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
        out[tid] = tid < 6 ? (float)v : posenc[(size_t)row * 8 + (tid - 6)];
    }
}

// One 32 x 32 tile of edges per workgroup: the column-side ranks, stored [j][i], are transposed through LDS.
__global__ void __launch_bounds__(kTile * 8)
gf_edge_kernel(const double *C, const double *u, const double *stat, const int *rank, float *edge, int n, int batch)
{
    __shared__ int tile[kTile][kTile + 1];
    const int b = blockIdx.z;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const size_t bnn = (size_t)b * n * n;
    const int *rank0 = rank + bnn;
    const int *rank1 = rank + ((size_t)batch * n * n + bnn);
    const double *st0 = stat + (size_t)b * n * kStats;
    const double *st1 = stat + ((size_t)batch + b) * n * kStats;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < n && j < n) tile[r][threadIdx.x] = rank1[(size_t)j * n + i];
    }
    __syncthreads();
    const double rden = n > 1 ? (double)(n - 1) : 1.0;
    for (int r = threadIdx.y; r < kTile; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i >= n || j >= n) continue;
        const double c = C[bnn + (size_t)i * n + j];
        const double *ri = st0 + (size_t)i * kStats, *cj = st1 + (size_t)j * kStats;
        float f[kEdgeFeatureDim];
        f[0] = (float)((c - ri[0]) / ri[1]);
        f[1] = (float)((double)rank0[(size_t)i * n + j] / rden);
        f[2] = (float)((double)tile[threadIdx.x][r] / rden);
        f[3] = (float)(c - ri[2]);
        f[4] = (float)(c - cj[2]);
        f[5] = (float)ri[3];
        f[6] = (float)cj[3];
        f[7] = (float)ri[4];
        f[8] = (float)cj[4];
        f[9] = u ? (float)((c - u[(size_t)b * n + i]) - cj[5]) : 0.0f;
        float2 *o = reinterpret_cast<float2 *>(edge + (bnn + (size_t)i * n + j) * kEdgeFeatureDim);
#pragma unroll
        for (int k = 0; k < kEdgeFeatureDim / 2; ++k) o[k] = make_float2(f[2 * k], f[2 * k + 1]);
    }
}

int gf_npad(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

size_t graph_features_workspace_bytes(int batch, int n)
{
    if (batch < 1 || batch > kGraphMaxBatch || n < 1 || n > kGraphMaxN) return 0;
    return graph_layout(nullptr, batch, n).bytes;
}

hipError_t launch_graph_features(const GraphFeatureParams &p, void *ws, hipStream_t stream)
{
    const GraphWs w = graph_layout(ws, p.batch, p.n);
    const int n = p.n, npad = gf_npad(n);
    const int tiles = (n + kTile - 1) / kTile;
    const dim3 tgrid(tiles, tiles, p.batch), tblock(kTile, 8);
    hipLaunchKernelGGL(gf_transpose_kernel, tgrid, tblock, 0, stream, p.C, w.Ct, n);
    const size_t lds = (size_t)npad * (8 + 8 + 4) + kGfThreads * 8;
    // once per process, and always the limit of the largest n, never this call's size: later calls with another n
    // then need no further host call (and none inside a capture)
    constexpr int kMaxLds = kGraphMaxN * (8 + 8 + 4) + kGfThreads * 8;
    static std::atomic<bool> raised{false};
    if (!raised.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gf_row_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
        if (e != hipSuccess) return e;
        raised.store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(gf_row_kernel, dim3(n, 2 * p.batch), dim3(kGfThreads), lds, stream, p.C, w.Ct, p.u, p.posenc,
                       p.row_out, p.col_out, w.stat, w.rank, n, npad, p.batch);
    hipLaunchKernelGGL(gf_edge_kernel, tgrid, tblock, 0, stream, p.C, p.u, w.stat, w.rank, p.edge, n, p.batch);
    return hipGetLastError();
}

}  // namespace lapwarm
