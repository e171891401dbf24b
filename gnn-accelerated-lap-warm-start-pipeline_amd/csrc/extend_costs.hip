// extend_costs.hip -- rectangular and cost-limited lapjv around the cold solver, gfx950, fp64.
//
// Reference: LAP/_lapjv_cpp/_lapjv.pyx:77-95 (the square matrix E the reference builds before
// lapjv_internal) and :115-124 (what it does with x, y afterwards).  Two kernels:
//   * extend: C [B][n_rows][n_cols] -> E [B][n][n].  E[:n_rows, :n_cols] = C; the rest is
//     `fill` (cost_limit / 2., computed by the host in fp64; 0 when there is no limit) except the
//     block E[n_rows:, n_cols:], which is 0.  A pure streaming kernel: one workgroup per row of E,
//     16-byte stores, 16-byte loads where the source row allows them.
//   * finish: the solver's x, y [B][n] -> the caller's x [B][n_rows], y [B][n_cols] with -1 for
//     "unmatched", the number of matched rows and opt = sum of C[i][x_i] over the matched rows in
//     row order, summed as numpy sums the compacted vector (pairwise_sum, device_utils.hpp).
#include "device_utils.hpp"
#include "extend_costs.hpp"

namespace lapwarm {

namespace {

constexpr int kExtThreads = 256;

// One workgroup per row r of E.  Element offsets inside E are even <=> 16-byte aligned (the
// workspace block is), so a row that starts on an odd offset gets one scalar head element and,
// when what is left is odd, one scalar tail; everything between is double2 stores.  A pair's
// source in C is read as one double2 when it lies inside the row of C on an even offset of a
// 16-byte aligned C, else as two doubles; the pair that straddles column n_cols is built by element.
__global__ void __launch_bounds__(kExtThreads)
extend_costs_kernel(const double *C, int n_rows, int n_cols, int n, double fill, int c_aligned, double *E)
{
    const int b = blockIdx.y, r = blockIdx.x;
    const size_t e0 = ((size_t)b * n + r) * n;
    double *erow = E + e0;
    const bool top = r < n_rows;
    const size_t c0 = ((size_t)b * n_rows + (top ? r : 0)) * n_cols;
    const double *crow = C + c0;
    const double right = top ? fill : 0.0;  // columns n_cols .. n - 1
    auto elem = [&](int j) -> double { return j < n_cols ? (top ? crow[j] : fill) : right; };
    const int head = (int)(e0 & 1);
    const int npairs = (n - head) >> 1;
    const bool src16 = c_aligned && ((c0 + head) & 1) == 0;
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

// One workgroup per instance.  Thread t owns the rows [t * per, (t + 1) * per): it counts its
// matched rows, thread 0 turns the counts into offsets, and every thread writes its gathered costs
// at its offset: the compacted vector in row order, which thread 0 then sums.
__global__ void __launch_bounds__(kExtThreads)
extended_finish_kernel(const double *C, int n_rows, int n_cols, int n, const int *xs, const int *ys,
                       const int *ret, int *x, int *y, double *opt, int *matched, double *gath)
{
    __shared__ int off[kExtThreads + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *xb = x + (size_t)b * n_rows, *yb = y + (size_t)b * n_cols;
    if (ret[b] != 0) {
        for (int i = tid; i < n_rows; i += kExtThreads) xb[i] = -1;
        for (int j = tid; j < n_cols; j += kExtThreads) yb[j] = -1;
        if (tid == 0) {
            if (opt) opt[b] = __longlong_as_double(0x7ff8000000000000LL);
            if (matched) matched[b] = 0;
        }
        return;
    }
    const int *xsb = xs + (size_t)b * n, *ysb = ys + (size_t)b * n;
    for (int j = tid; j < n_cols; j += kExtThreads) {
        const int i = ysb[j];
        yb[j] = ((unsigned)i >= (unsigned)n_rows) ? -1 : i;
    }
    const int per = (n_rows + kExtThreads - 1) / kExtThreads;
    const int i0 = (tid * per < n_rows) ? tid * per : n_rows;
    const int i1 = (i0 + per < n_rows) ? i0 + per : n_rows;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) {
        const int j = xsb[i];
        const int xo = ((unsigned)j >= (unsigned)n_cols) ? -1 : j;
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
    double *g = gath + (size_t)b * n_rows;
    const double *Cb = C + (size_t)b * n_rows * n_cols;
    int q = off[tid];
    for (int i = i0; i < i1; ++i) {
        const int j = xsb[i];
        if ((unsigned)j < (unsigned)n_cols) g[q++] = Cb[(size_t)i * n_cols + j];
    }
    __syncthreads();
    // np.sum starts from +0.0: an empty or all -0.0 vector sums to +0.0
    if (tid == 0) opt[b] = 0.0 + pairwise_sum<10>(g, total);
}

}  // namespace

hipError_t launch_extend_costs(const double *C, int batch, int n_rows, int n_cols, int n, double fill, double *E,
                               hipStream_t stream)
{
    const int c_aligned = (reinterpret_cast<uintptr_t>(C) % 16) == 0;
    hipLaunchKernelGGL(extend_costs_kernel, dim3(n, batch), dim3(kExtThreads), 0, stream, C, n_rows, n_cols, n,
                       fill, c_aligned, E);
    return hipGetLastError();
}

hipError_t launch_extended_finish(const double *C, int batch, int n_rows, int n_cols, int n, const int *xs,
                                  const int *ys, const int *ret, int *x, int *y, double *opt, int *matched,
                                  double *gath, hipStream_t stream)
{
    hipLaunchKernelGGL(extended_finish_kernel, dim3(batch), dim3(kExtThreads), 0, stream, C, n_rows, n_cols, n, xs,
                       ys, ret, x, y, opt, matched, gath);
    return hipGetLastError();
}

}  // namespace lapwarm
