// extend_ragged.hip -- cold lapjv of a batch of different sizes and shapes, gfx950, fp64: the kernels around the
// ragged launches of jv_instance_kernel (jv_solver.hip) with mode = kModeCold.
//
// Reference: LAP/_lapjv_cpp/_lapjv.pyx:77-95 and :115-124, per instance; extend_costs.hip is the same for one
// shape per call, and the extend and finish kernels here keep its structure.  Four kernels:
//   * init (square batches, lapwarm_lapjv_ragged): x, y -1, ret 2, stats 0;
//   * shapes: one workgroup turns the device shapes and limits into the extended sizes n_b and the offsets of
//     the packed E_b (an exclusive scan of n_b^2), so that the entry point never reads the device;
//   * extend: grid (largest n, batch), one workgroup per row of an E_b, 16-byte stores;
//   * finish: one workgroup per instance, as extended_finish_kernel.
#include <math.h>
#include <stdint.h>

#include "device_utils.hpp"
#include "extend_ragged.hpp"
#include "jv_solver.hpp"

namespace lapwarm {

namespace {

constexpr int kExtThreads = 256;

__global__ void __launch_bounds__(kExtThreads)
lapjv_ragged_init_kernel(long long *x, long long *y, int *ret, long long *stats, int N)
{
    const int b = blockIdx.y, j = blockIdx.x * kExtThreads + threadIdx.x;
    if (j < N) {
        x[(size_t)b * N + j] = -1;
        y[(size_t)b * N + j] = -1;
    }
    if (j == 0) ret[b] = 2;
    if (stats && j < kStatsPerInstance) stats[(size_t)b * kStatsPerInstance + j] = 0;
}

// n_b as lapwarm_lapjv_extended_n, or 0 for a shape the host did not plan for (ExtRagged)
__device__ __forceinline__ int extended_size(const ExtRagged &g, int b)
{
    const int r = g.n_rows[b], c = g.n_cols[b];
    if (r < 1 || c < 1 || r > g.R || c > g.Q || (g.ld > 0 && c > g.ld)) return 0;
    if (r != c && !g.extend_cost) return 0;
    const long long n = (g.limits[b] < (double)INFINITY) ? (long long)r + c : (r > c ? r : c);
    return n <= g.N ? (int)n : 0;
}

// Thread t owns the instances [t * per, (t + 1) * per): it sums their n_b^2, thread 0 turns the sums into
// offsets, and every thread walks its instances again.  An E_b that would end beyond e_total is dropped (its
// place stays unused): the offsets of the others are those of the host's plan whenever the shapes are.
__global__ void __launch_bounds__(kExtThreads) extend_shapes_kernel(ExtRagged g)
{
    __shared__ long long base[kExtThreads + 1];
    const int tid = threadIdx.x;
    const int per = (g.batch + kExtThreads - 1) / kExtThreads;
    const int b0 = (tid * per < g.batch) ? tid * per : g.batch;
    const int b1 = (b0 + per < g.batch) ? b0 + per : g.batch;
    long long sum = 0;
    for (int b = b0; b < b1; ++b) {
        const long long n = extended_size(g, b);
        sum += n * n;
    }
    base[tid + 1] = sum;
    __syncthreads();
    if (tid == 0) {
        base[0] = 0;
        for (int t = 0; t < kExtThreads; ++t) base[t + 1] += base[t];
    }
    __syncthreads();
    long long off = base[tid];
    for (int b = b0; b < b1; ++b) {
        long long n = extended_size(g, b);
        if (off + n * n > g.e_total) n = 0;
        g.e_n[b] = (int)n;
        g.e_off[b] = off;
        off += n * n;
    }
}

// One workgroup per row r of E_b; workgroups with r >= n_b leave.  Element offsets inside the E area are even
// <=> 16-byte aligned, so a row that starts on an odd offset (odd n_b and odd r, or an E_b behind an odd number
// of elements) gets one scalar head element and, when what is left is odd, one scalar tail; everything between
// is double2 stores.  A pair's source in C is read as one double2 when it lies inside the row of C on a 16-byte
// aligned address, else as two doubles; the pair that straddles column n_cols is built by element.
__global__ void __launch_bounds__(kExtThreads) extend_ragged_kernel(ExtRagged g, int *ret, long long *stats)
{
    const int b = blockIdx.y, r = blockIdx.x;
    if (r == 0) {  // what the instance keeps when no solver launch takes it
        if (threadIdx.x == 0) ret[b] = 2;
        if (stats && threadIdx.x < kStatsPerInstance) stats[(size_t)b * kStatsPerInstance + threadIdx.x] = 0;
    }
    const int n = g.e_n[b];
    if (r >= n) return;
    const int n_rows = g.n_rows[b], n_cols = g.n_cols[b];
    const double limit = g.limits[b];
    const double fill = (limit < (double)INFINITY) ? limit / 2. : 0.0;  // (exact: the host would get the same)
    const size_t e0 = (size_t)g.e_off[b] + (size_t)r * n;
    double *erow = g.E + e0;
    const bool top = r < n_rows;
    const double *crow = g.C + g.offsets[b] + (size_t)(top ? r : 0) * (size_t)(g.ld ? g.ld : n_cols);
    const double right = top ? fill : 0.0;  // columns n_cols .. n - 1
    auto elem = [&](int j) -> double { return j < n_cols ? (top ? crow[j] : fill) : right; };
    const int head = (int)(e0 & 1);
    const int npairs = (n - head) >> 1;
    const bool src16 = (reinterpret_cast<uintptr_t>(crow + head) & 15) == 0;
    if (threadIdx.x == 0) {
        if (head) erow[0] = elem(0);
        if ((n - head) & 1) erow[n - 1] = elem(n - 1);
    }
    const int ncopy = top ? n_cols : 0;
    for (int k = threadIdx.x; k < npairs; k += kExtThreads) {
        const int j = head + 2 * k;
        double2 o;
        if (j + 1 < ncopy) {
            if (src16) {
                o = *reinterpret_cast<const double2 *>(crow + j);
            } else {
                o.x = crow[j];
                o.y = crow[j + 1];
            }
        } else {
            o.x = elem(j);
            o.y = elem(j + 1);
        }
        *reinterpret_cast<double2 *>(erow + j) = o;
    }
}

// One workgroup per instance.  Thread t owns the rows [t * per, (t + 1) * per): it counts its matched rows,
// thread 0 turns the counts into offsets, and every thread writes its gathered costs at its offset: the
// compacted vector in row order, which thread 0 then sums.
__global__ void __launch_bounds__(kExtThreads)
extended_finish_ragged_kernel(ExtRagged g, const long long *xs, const long long *ys, const int *ret, int *x, int *y,
                              double *opt, int *matched, double *gath)
{
    __shared__ int off[kExtThreads + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *xb = x + (size_t)b * g.R, *yb = y + (size_t)b * g.Q;
    const int n = g.e_n[b];
    if (ret[b] != 0 || n == 0) {
        for (int i = tid; i < g.R; i += kExtThreads) xb[i] = -1;
        for (int j = tid; j < g.Q; j += kExtThreads) yb[j] = -1;
        if (tid == 0) {
            if (opt) opt[b] = __longlong_as_double(0x7ff8000000000000LL);
            if (matched) matched[b] = 0;
        }
        return;
    }
    const int n_rows = g.n_rows[b], n_cols = g.n_cols[b];
    const long long *xsb = xs + (size_t)b * g.N, *ysb = ys + (size_t)b * g.N;
    for (int j = tid; j < g.Q; j += kExtThreads) {
        const long long i = (j < n_cols) ? ysb[j] : -1;
        yb[j] = ((unsigned long long)i >= (unsigned long long)n_rows) ? -1 : (int)i;
    }
    for (int i = n_rows + tid; i < g.R; i += kExtThreads) xb[i] = -1;
    const int per = (n_rows + kExtThreads - 1) / kExtThreads;
    const int i0 = (tid * per < n_rows) ? tid * per : n_rows;
    const int i1 = (i0 + per < n_rows) ? i0 + per : n_rows;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) {
        const long long j = xsb[i];
        const int xo = ((unsigned long long)j >= (unsigned long long)n_cols) ? -1 : (int)j;
        xb[i] = xo;
        cnt += (xo != -1);
    }
    off[tid + 1] = cnt;
    __syncthreads();
    if (tid == 0) {
        off[0] = 0;
        for (int t = 0; t < kExtThreads; ++t) off[t + 1] += off[t];
    }
    __syncthreads();
    const int total = off[kExtThreads];
    if (tid == 0 && matched) matched[b] = total;
    if (!opt) return;
    double *gb = gath + (size_t)b * g.R;
    const double *Cb = g.C + g.offsets[b];
    const size_t ldc = (size_t)(g.ld ? g.ld : n_cols);
    int q = off[tid];
    for (int i = i0; i < i1; ++i) {
        const long long j = xsb[i];
        if ((unsigned long long)j < (unsigned long long)n_cols) gb[q++] = Cb[(size_t)i * ldc + (size_t)j];
    }
    __syncthreads();
    // np.sum starts from +0.0: an empty or all -0.0 vector sums to +0.0
    if (tid == 0) opt[b] = 0.0 + pairwise_sum<10>(gb, total);
}

bool bad_dims(const ExtRagged &g)
{
    return g.batch < 1 || g.batch > 65535 || g.N < 1 || g.N > 16384 || g.R < 1 || g.Q < 1 || g.ld < 0;
}

}  // namespace

hipError_t launch_lapjv_ragged_init(long long *x, long long *y, int *ret, long long *stats, int batch, int N,
                                    hipStream_t stream)
{
    if (batch < 1 || batch > 65535 || N < 1 || N > 16384) return hipErrorInvalidValue;
    // (at least kStatsPerInstance threads per instance: one workgroup of 256 has them)
    hipLaunchKernelGGL(lapjv_ragged_init_kernel, dim3((N + kExtThreads - 1) / kExtThreads, batch), dim3(kExtThreads),
                       0, stream, x, y, ret, stats, N);
    return hipGetLastError();
}

hipError_t launch_extend_shapes(const ExtRagged &g, hipStream_t stream)
{
    if (bad_dims(g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extend_shapes_kernel, dim3(1), dim3(kExtThreads), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_extend_costs_ragged(const ExtRagged &g, int *ret, long long *stats, hipStream_t stream)
{
    if (bad_dims(g) || (reinterpret_cast<uintptr_t>(g.E) & 15) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extend_ragged_kernel, dim3(g.N, g.batch), dim3(kExtThreads), 0, stream, g, ret, stats);
    return hipGetLastError();
}

hipError_t launch_extended_finish_ragged(const ExtRagged &g, const long long *xs, const long long *ys, const int *ret,
                                         int *x, int *y, double *opt, int *matched, double *gath, hipStream_t stream)
{
    if (bad_dims(g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extended_finish_ragged_kernel, dim3(g.batch), dim3(kExtThreads), 0, stream, g, xs, ys, ret, x,
                       y, opt, matched, gath);
    return hipGetLastError();
}

}  // namespace lapwarm
