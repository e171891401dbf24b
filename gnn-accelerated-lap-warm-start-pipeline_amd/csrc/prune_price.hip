// prune_price.hip -- per-row selection over dense rows that emits CSR, gfx950: the grow step of the pruned exact
// solve ("Exact dense LAP through sparse LAPMOD").
//
// Workgroup (i, b) owns row i of instance b and holds it in registers: thread t has the columns t, t + T, t + 2T,
// ... (at most kPruneItems of them, T = blockDim.x), as the order-preserving 64-bit image of key_ij = C_ij - key_j.
// An entry is eligible when it is absent from the row (a bitmap of n bits in LDS, set from the row's current
// columns; the diagonal alone when there is no current CSR) and its key is below the row's bound.  Where more than m
// entries are eligible an 8 x 8-bit radix select over the images finds the image of the m-th smallest key and how
// many of its ties are taken; the entries taken are then the eligible ones with a smaller image, and the first
// `ties` in column order with that image.  The emit pass walks the row in column order, T columns at a time, and
// gives every column that is present or taken its position by a workgroup prefix count: the merged row comes out
// sorted, and its values are read from C (a present entry's value is C_ij too).
//
// The count pass does the selection and leaves (image, ties, length) per row; one workgroup per instance turns the
// lengths into row starts and reduces viol, added and ret; the fill pass recomputes the images and emits with the
// stored threshold.  Integer LDS atomics only (histogram and bitmap): equal inputs give equal bits.
#include "device_utils.hpp"
#include "prune_price.hpp"

namespace lapwarm {

namespace {

constexpr int kScanThreads = 256;

// Order-preserving image of a double: a < b <=> image(a) < image(b), -0.0 and +0.0 share one image, and every NaN
// has the largest (after +inf).
__device__ __forceinline__ unsigned long long key_image(double x)
{
    if (x != x) return ~0ull;
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (b == 0x8000000000000000ull) b = 0ull;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool finite_f64(double x)
{
    return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// Workgroup prefix count: the exclusive prefix of v over the threads and the total.  One barrier; the two slot
// sets alternate as in BlockExchange.
struct BlockScan {
    int (*slots)[kMaxWaves];
    int lane, wave, nwaves, parity;

    __device__ __forceinline__ int excl(int v, int *total)
    {
        const int incl = wave_incl_prefix_sum_i32(v);
        if (lane == kWave - 1) slots[parity][wave] = incl;
        __syncthreads();
        int base = 0, tot = 0;
        for (int w = 0; w < nwaves; ++w) {
            const int s = slots[parity][w];
            base += (w < wave) ? s : 0;
            tot += s;
        }
        parity ^= 1;
        *total = tot;
        return base + incl - v;
    }
    __device__ __forceinline__ int sum(int v)
    {
        int total;
        excl(v, &total);
        return total;
    }
};

template <bool FILL>
__global__ void __launch_bounds__(kPruneMaxThreads) prune_row_kernel(RaggedBatch g, PruneGrow p, PruneWs w)
{
    __shared__ unsigned present[kMaxN / 32];
    __shared__ int hist[256];
    __shared__ int slots[2][kMaxWaves];
    __shared__ int sel[2];
    const int b = blockIdx.y, i = blockIdx.x;
    const int n = uni(ragged_size(g, b));
    if (i >= n) return;
    if constexpr (FILL) {
        if (p.ret[b] != kPruneOk) return;
    }
    const int T = blockDim.x, tid = threadIdx.x;
    BlockScan scan{slots, tid & (kWave - 1), tid >> 6, T >> 6, 0};
    const size_t o = (size_t)b * g.N + i;
    const size_t stride = g.ld ? g.ld : n;
    const double *row = g.C + g.offsets[b] + (size_t)i * stride;
    const double *keyb = p.key ? p.key + (size_t)b * g.N : nullptr;

    // the columns the row holds now
    for (int q = tid; q < (n + 31) / 32; q += T) present[q] = 0u;
    __syncthreads();
    int bad = 0;
    if (p.kk_in) {
        const int *ii = p.ii_in + p.row_off_in[b];
        const int lo = ii[i], hi = ii[i + 1];
        if (lo < 0 || hi < lo || hi - lo > n) {
            bad = 1;
        } else {
            const int *kk = p.kk_in + p.nnz_off_in[b];
            for (int e = lo + tid; e < hi; e += T) {
                const int c = kk[e];
                if ((unsigned)c < (unsigned)n)
                    atomicOr(&present[c >> 5], 1u << (c & 31));
                else
                    bad = 1;
            }
        }
    } else if (tid == 0) {
        present[i >> 5] = 1u << (i & 31);
    }
    __syncthreads();

    double bound = pos_inf();
    if (p.x) {
        const int xi = p.x[o];
        if ((unsigned)xi < (unsigned)n) {
            bound = row[xi] - keyb[xi];
        } else {
            bad = 1;
            bound = -pos_inf();
        }
    }

    unsigned long long img[kPruneItems];
    unsigned elig = 0u, pres = 0u;
#pragma unroll
    for (int q = 0; q < kPruneItems; ++q) {
        const int j = tid + q * T;
        img[q] = ~0ull;
        if (j < n) {
            const double c = row[j];
            const double kj = keyb ? keyb[j] : 0.0;
            const double kv = keyb ? c - kj : c;
            if (!(c >= 0.0 && c < kLarge) || !finite_f64(kj)) bad = 1;
            const bool here = (present[j >> 5] >> (j & 31)) & 1u;
            if (here) pres |= 1u << q;
            if (!here && kv < bound) elig |= 1u << q;
            img[q] = key_image(kv);
        }
    }

    unsigned long long thr;
    int ties;
    if constexpr (FILL) {
        thr = w.thr[o];
        ties = w.ties[o];
    } else {
        const int n_elig = scan.sum(__popc(elig));
        bad = scan.sum(bad);
        thr = ~0ull;
        ties = 0x7fffffff;
        if (n_elig > p.m) {  // workgroup-uniform
            unsigned long long prefix = 0ull;
            int need = p.m;
            for (int pass = 0; pass < 8; ++pass) {
                const int shift = 56 - 8 * pass;
                for (int h = tid; h < 256; h += T) hist[h] = 0;
                __syncthreads();
#pragma unroll
                for (int q = 0; q < kPruneItems; ++q) {
                    const unsigned long long above = pass ? (img[q] >> (shift + 8)) : 0ull;
                    if (((elig >> q) & 1u) && above == prefix) atomicAdd(&hist[(int)((img[q] >> shift) & 255ull)], 1);
                }
                __syncthreads();
                if (scan.wave == 0) {  // lane l owns the bins 4l .. 4l + 3
                    const int c0 = hist[4 * scan.lane], c1 = hist[4 * scan.lane + 1], c2 = hist[4 * scan.lane + 2];
                    const int s = c0 + c1 + c2 + hist[4 * scan.lane + 3];
                    const int incl = wave_incl_prefix_sum_i32(s);
                    const int excl = incl - s;
                    if (excl < need && need <= incl) {  // one lane
                        int r = need - excl, d = 4 * scan.lane;
                        if (r > c0) {
                            r -= c0;
                            ++d;
                            if (r > c1) {
                                r -= c1;
                                ++d;
                                if (r > c2) {
                                    r -= c2;
                                    ++d;
                                }
                            }
                        }
                        sel[0] = d;
                        sel[1] = r;
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | (unsigned long long)sel[0];
                need = sel[1];
            }
            thr = prefix;
            ties = need;
        }
        if (tid == 0) {
            w.thr[o] = thr;
            w.ties[o] = ties;
            w.nelig[o] = n_elig;
            w.bad[o] = bad;
        }
    }

    // the merged row in column order, T columns at a time
    const bool all = thr == ~0ull && ties == 0x7fffffff;  // every eligible entry is taken: no tie ranks needed
    long long out0 = 0;
    int row_len = 0;
    if constexpr (FILL) {
        const int *ii = p.ii_out + p.row_off_out[b];
        out0 = p.nnz_off_out[b] + ii[i];
        row_len = ii[i + 1] - ii[i];
    }
    const int chunks = (n + T - 1) / T;
    int tie_base = 0, out_base = 0;
#pragma unroll
    for (int q = 0; q < kPruneItems; ++q) {
        if (q < chunks) {  // workgroup-uniform
            const bool e = (elig >> q) & 1u;
            bool take = e;
            if (!all) {
                const bool tie = e && img[q] == thr;
                int tie_total;
                const int rank = tie_base + scan.excl(tie ? 1 : 0, &tie_total);
                tie_base += tie_total;
                take = e && (img[q] < thr || (tie && rank < ties));
            }
            const bool out = take || ((pres >> q) & 1u);
            int out_total;
            const int pos = out_base + scan.excl(out ? 1 : 0, &out_total);
            out_base += out_total;
            if constexpr (FILL) {
                if (out && pos < row_len) {
                    const int j = tid + q * T;
                    p.kk_out[out0 + pos] = j;
                    p.cc_out[out0 + pos] = row[j];
                }
            }
        }
    }
    if constexpr (!FILL) {
        if (tid == 0) w.len[o] = out_base;
    }
}

// Row starts of the next CSR, and viol, added and ret of the instance: one workgroup per instance.
__global__ void __launch_bounds__(kScanThreads) prune_scan_kernel(RaggedBatch g, PruneGrow p, PruneWs w)
{
    __shared__ int slots[2][kMaxWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = uni(ragged_size(g, b));
    if (n == 0) {
        if (tid == 0) {
            p.added[b] = 0;
            p.viol[b] = 0;
            p.ret[b] = kPruneEmpty;
        }
        return;
    }
    BlockScan scan{slots, tid & (kWave - 1), tid >> 6, kScanThreads >> 6, 0};
    int *ii = p.cc_out ? p.ii_out + p.row_off_out[b] : nullptr;
    int base = 0, viol = 0, bad = 0;  // viol <= n * n < 2^31
    for (int i0 = 0; i0 < n; i0 += kScanThreads) {
        const int i = i0 + tid;
        const size_t o = (size_t)b * g.N + i;
        const int len = (i < n) ? w.len[o] : 0;
        if (i < n) {
            viol += w.nelig[o];
            bad |= w.bad[o];
        }
        int total;
        const int start = base + scan.excl(len, &total);
        if (ii && i < n) ii[i] = start;
        base += total;
    }
    viol = scan.sum(viol);
    bad = scan.sum(bad);
    if (tid == 0) {
        if (ii) ii[n] = base;
        const long long nnz_in = p.kk_in ? p.ii_in[p.row_off_in[b] + n] : 0;
        p.added[b] = (long long)base - nnz_in;
        p.viol[b] = viol;
        p.ret[b] = bad ? kPruneInadmissible : (p.cc_out && base > p.cap_out[b]) ? kPruneNoRoom : kPruneOk;
    }
}

constexpr int kFinishChunk = 2048;

// u, cost and the zeroed tails: one workgroup per instance.  The cost is summed serially in ascending i by one
// thread, from values the workgroup gathers kFinishChunk at a time.
__global__ void __launch_bounds__(kScanThreads)
prune_finish_kernel(RaggedBatch g, const int *x, double *v, const int *ret, double *u, double *cost)
{
    __shared__ double vals[kFinishChunk];
    __shared__ int bad_any;
    const int b = blockIdx.x, tid = threadIdx.x, N = g.N;
    const int n = uni(ragged_size(g, b));
    const int r = ret[b];
    double *ub = u + (size_t)b * N, *vb = v + (size_t)b * N;
    if (n == 0 || (r != 0 && r != 2)) {
        for (int j = tid; j < N; j += kScanThreads) ub[j] = vb[j] = 0.0;
        if (tid == 0) cost[b] = pos_inf();
        return;
    }
    if (tid == 0) bad_any = 0;
    const size_t stride = g.ld ? g.ld : n;
    const double *base = g.C + g.offsets[b];
    const int *xb = x + (size_t)b * N;
    double total = 0.0;
    for (int i0 = 0; i0 < n; i0 += kFinishChunk) {
        __syncthreads();
        for (int i = i0 + tid; i < n && i < i0 + kFinishChunk; i += kScanThreads) {
            const int xi = xb[i];
            double c = 0.0, ui = 0.0;
            if ((unsigned)xi < (unsigned)n) {
                c = base[(size_t)i * stride + xi];
                ui = c - vb[xi];
            } else {
                bad_any = 1;
            }
            vals[i - i0] = c;
            ub[i] = ui;
        }
        __syncthreads();
        if (tid == 0) {
            const int m = (n - i0 < kFinishChunk) ? n - i0 : kFinishChunk;
            for (int q = 0; q < m; ++q) total = total + vals[q];
        }
    }
    for (int j = n + tid; j < N; j += kScanThreads) ub[j] = vb[j] = 0.0;
    if (tid == 0) cost[b] = bad_any ? pos_inf() : total;
}

}  // namespace

hipError_t launch_prune_grow(const RaggedBatch &g, const PruneGrow &p, const PruneWs &w, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N) || p.m < 1 || p.m > kPruneMaxM) return hipErrorInvalidValue;
    int threads = ((g.N + 7) / 8 + kWave - 1) / kWave * kWave;  // up to 8 columns a thread below 8192
    if (threads > kPruneMaxThreads) threads = kPruneMaxThreads;
    const dim3 grid(g.N, g.batch);
    hipLaunchKernelGGL(prune_row_kernel<false>, grid, dim3(threads), 0, stream, g, p, w);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(g.batch), dim3(kScanThreads), 0, stream, g, p, w);
    if (p.cc_out) hipLaunchKernelGGL(prune_row_kernel<true>, grid, dim3(threads), 0, stream, g, p, w);
    return hipGetLastError();
}

hipError_t launch_prune_finish(const RaggedBatch &g, const int *x, double *v, const int *ret, double *u, double *cost,
                               hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prune_finish_kernel, dim3(g.batch), dim3(kScanThreads), 0, stream, g, x, v, ret, u, cost);
    return hipGetLastError();
}

}  // namespace lapwarm
