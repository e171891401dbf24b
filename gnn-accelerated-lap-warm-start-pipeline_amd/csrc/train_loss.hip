// train_loss.hip -- the OneGNN training loss on the device, gfx950, float32 terms with fp64 sums.
//
// Reference: gnn/train_one_gnn.py:180-226 `compute_loss` with its host greedy `greedy_primal_upper`
// (:137-177).  Per instance b with n_b = sizes[b] valid rows and columns (a prefix of the padded n):
//   v_j        = min_i (C_ij - u_i), a_j the lowest row attaining it
//   dual_lower = sum_i u_i + sum_j v_j
//   feas       = sum_ij relu((u_i + v_j) - C_ij) / n_b^2
//   u_reg      = sum_i (u_i - u_target_i)^2 / n_b
//   primal_upper = cost of the greedy assignment on reduced_ij = (C_ij - u_i) - v_j: rows in ascending
//                  order of min_j reduced_ij, each takes its cheapest column not yet used
// Every float32 term is formed as the reference forms it (this file is built with -ffp-contract=off);
// every sum is accumulated in fp64 in a fixed order and rounded to float32 once.  Ties go to the lowest
// index everywhere (a_j, the row order, the column a row takes): the reference leaves them to an
// unstable np.argsort.
//
// What runs here, all on the caller's stream:
//   * column pass: lanes along j, a chunk of rows per workgroup, (value, row) partials combined by a
//     second kernel, which also clears the counters of the call;
//   * hinge pass, one read of C: a wave per row with lanes along j gives sum h (fp64 partial per wave),
//     R_i, m_i = min_j reduced_ij with its lowest j; K_j is an int32 atomic per positive h (h is
//     rounding residue: positive on few elements);
//   * one workgroup per instance: cnt_i and sum_{a_j = i} K_j by integer scatter, the O(n) sums, the
//     row order by a bitonic sort of (m_i, i) in LDS, the greedy with the used-column bitmap in LDS,
//     primal_upper, the four terms and ret;
//   * backward: one thread per (b, i), closed form in fp64 from cnt, R and the scattered K.
//
// The DualGNN loss (gnn/train.py:267-308 `compute_loss`) differs in its third term only:
//   v_reg = sum_j (vh_j - v_j)^2 / n_b,  vh = the model's v_hint
// which sends 2 d_j / n_b, d_j = vh_j - v_j, into vh_j and, through v_j = C_{a_j j} - u_{a_j}, 2 S_i / n_b into
// u_i with S_i = sum_{a_j = i} d_j.  The column pass, the hinge pass and the greedy are shared; the workgroup of
// an instance forms S_i without floating-point atomics: a bitonic sort of (a_j << 32 | j) in the LDS buffer the
// row order uses afterwards, then one serial fp64 sum per run of equal a_j, which adds in ascending j.
#include "device_utils.hpp"
#include "dense_sweeps.hpp"  // colmin_chunks
#include "train_loss.hpp"

namespace lapwarm {

namespace {

constexpr int kTlThreads = 256;                             // column and hinge passes
constexpr int kTlWaves = kTlThreads / kWave;
constexpr int kTlGreedyThreads = 1024;
constexpr int kTlEpt = kTrainLossMaxN / kTlGreedyThreads;   // rows per thread of the greedy workgroup

__device__ __forceinline__ float f32_inf() { return __uint_as_float(0x7f800000u); }
__device__ __forceinline__ float f32_nan() { return __uint_as_float(0x7fc00000u); }
// n_b, or 0 for a size outside 1..n: such an instance has no valid row in any pass
__device__ __forceinline__ int tl_size(int s, int n) { return (s >= 1 && s <= n) ? s : 0; }
__device__ __forceinline__ unsigned long long tl_pack(float val, int idx)
{
    return ((unsigned long long)f32_key(val) << 32) | (unsigned)idx;
}

// ------------------------------------------------------------------------------------------
// Column pass, part 1: grid (column tiles, chunks, batch), W columns per lane (W = 4: 16 B loads).
// torch.min propagates NaN: a NaN replaces the running minimum and stays.
// ------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kTlThreads) tl_colmin_partial_kernel(TrainLossParams p, int rows_per)
{
    const int b = blockIdx.z, chunk = blockIdx.y, n = p.n;
    const int nb = tl_size(p.sizes[b], n);
    const int j = (blockIdx.x * kTlThreads + threadIdx.x) * W;
    if (j >= nb) return;
    const int i0 = chunk * rows_per;
    const int i1 = (i0 + rows_per < nb) ? i0 + rows_per : nb;
    const float *base = p.C + (size_t)b * n * n + j;
    const float *ub = p.u + (size_t)b * n;
    float m[W];
    int a[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
        m[e] = f32_inf();
        a[e] = 0x7fffffff;
    }
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const float ui = ub[i];
        float c[W];
        if constexpr (W == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(base + (size_t)i * n);
            c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
        } else {
            c[0] = base[(size_t)i * n];
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float t = c[e] - ui;
            if (t < m[e] || t != t) {
                m[e] = t;
                a[e] = i;
            }
        }
    }
    const size_t po = ((size_t)b * p.chunks + chunk) * n + j;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        p.pval[po + e] = m[e];
        p.parg[po + e] = a[e];
    }
}

// Part 2: grid (column blocks, batch), one thread per (b, j).  Chunks hold ascending rows, so the strict
// compare keeps the lowest row.  Also clears K, cnt and ksum and sets assign to -1 for the call.
__global__ void __launch_bounds__(kTlThreads) tl_colmin_final_kernel(TrainLossParams p)
{
    const int b = blockIdx.y, n = p.n;
    const int j = blockIdx.x * kTlThreads + threadIdx.x;
    if (j >= n) return;
    const int nb = tl_size(p.sizes[b], n);
    const size_t o = (size_t)b * n + j;
    p.K[o] = 0;
    p.cnt[o] = 0;
    p.ksum[o] = 0;
    p.assign[o] = -1;
    float m = 0.0f;
    int arg = -1;
    if (j < nb) {
        m = f32_inf();
        arg = 0x7fffffff;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t po = ((size_t)b * p.chunks + c) * n + j;
            const float t = p.pval[po];
            if (t < m || t != t) {
                m = t;
                arg = p.parg[po];
            }
        }
        if (arg == 0x7fffffff) arg = 0;  // a column of +inf: argmin is row 0
    }
    p.v[o] = m;
    p.arow[o] = arg;
}

// ------------------------------------------------------------------------------------------
// Hinge pass: grid (row blocks, batch); wave w of block x owns rows [s * rows_per_wave, ...) with
// s = 4 x + w and scans each with lanes along j.
// ------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kTlThreads) tl_hinge_kernel(TrainLossParams p)
{
    const int b = blockIdx.y, n = p.n;
    const int nb = tl_size(p.sizes[b], n);
    const int lane = threadIdx.x & (kWave - 1);
    const int slot = blockIdx.x * kTlWaves + (threadIdx.x >> 6);
    const int r0 = slot * p.rows_per_wave;
    const int r1 = (r0 + p.rows_per_wave < nb) ? r0 + p.rows_per_wave : nb;
    const size_t bn = (size_t)b * n;
    const float *vb = p.v + bn;
    int *Kb = p.K + bn;
    double hs = 0.0;
    for (int i = r0; i < r1; ++i) {
        const float ui = p.u[bn + i];
        const float *row = p.C + (bn + i) * n;
        int rcnt = 0;
        float mv = f32_inf();
        int mjx = 0x7fffffff;
        for (int j = lane * W; j < nb; j += kWave * W) {
            float c[W], vj[W];
            if constexpr (W == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(row + j);
                const float4 w = *reinterpret_cast<const float4 *>(vb + j);
                c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
                vj[0] = w.x, vj[1] = w.y, vj[2] = w.z, vj[3] = w.w;
            } else {
                c[0] = row[j];
                vj[0] = vb[j];
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                if (W > 1 && j + e >= nb) break;
                const float red = (c[e] - ui) - vj[e];
                if (red < mv) {
                    mv = red;
                    mjx = j + e;
                }
                const float h = (ui + vj[e]) - c[e];
                if (!(h <= 0.0f)) {  // positive, or NaN as torch.relu passes it on
                    hs += (double)h;
                    if (h > 0.0f) {
                        ++rcnt;
                        atomicAdd(&Kb[j + e], 1);
                    }
                }
            }
        }
        const unsigned long long best = wave_reduce<MinU64>(tl_pack(mv, mjx));
        rcnt = wave_sum_i32(rcnt);
        if (lane == 0) {
            p.mkey[bn + i] = (unsigned)(best >> 32);
            p.mj[bn + i] = (int)(unsigned)best;
            p.R[bn + i] = rcnt;
        }
    }
    hs = wave_sum_f64(hs);
    if (lane == 0) p.hpart[(size_t)b * p.hparts + slot] = hs;
}

// ascending bitonic sort of ord[0 .. p2), p2 a power of two, by the whole workgroup; ends on a barrier
__device__ __forceinline__ void tl_bitonic_sort(unsigned long long *ord, int p2, int tid, int nt)
{
    for (int k = 2; k <= p2; k <<= 1) {
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < p2 / 2; t += nt) {
                const int lo = ((t & ~(s - 1)) << 1) | (t & (s - 1));
                const int hi = lo + s;
                const unsigned long long x = ord[lo], y = ord[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    ord[lo] = y;
                    ord[hi] = x;
                }
            }
            __syncthreads();
        }
    }
}

// S_i = sum_{j: a_j = i} d_j of the DualGNN loss into p.vsum, d_j = vh_j - v_j into p.dj.  ord[] is free here:
// it takes the keys (a_j << 32 | j), sorted; then every slot trades its j for the bits of d_j, and the thread
// at the head of a run of equal a_j adds the run in fp64, front to back: ascending j, whatever the run length.
// Rows that own no column keep the 0 written first.
__device__ __forceinline__ void tl_segment_sums(const TrainLossParams &p, unsigned long long *ord, int p2, size_t bn,
                                                int nb, int tid, int nt)
{
    const float *vhb = p.vh + bn, *vb = p.v + bn;
    for (int i = tid; i < nb; i += nt) p.vsum[bn + i] = 0.0;
    for (int j = tid; j < p2; j += nt) {
        unsigned long long key = ~0ull;
        if (j < nb) {
            p.dj[bn + j] = vhb[j] - vb[j];
            const int a = p.arow[bn + j];
            if ((unsigned)a < (unsigned)nb) key = ((unsigned long long)(unsigned)a << 32) | (unsigned)j;
        }
        ord[j] = key;
    }
    __syncthreads();  // the keys, and the zeros of vsum before any head stores its sum
    tl_bitonic_sort(ord, p2, tid, nt);
    for (int k = tid; k < nb; k += nt) {
        const unsigned long long e = ord[k];
        if (e != ~0ull) {
            const int j = (int)(unsigned)e;
            ord[k] = (e & 0xffffffff00000000ull) | __float_as_uint(vhb[j] - vb[j]);
        }
    }
    __syncthreads();
    for (int k = tid; k < nb; k += nt) {
        const unsigned long long e = ord[k];
        if (e == ~0ull) continue;
        const unsigned row = (unsigned)(e >> 32);
        if (k > 0 && (unsigned)(ord[k - 1] >> 32) == row) continue;  // not the head of its run
        double s = 0.0;
        for (int q = k; q < nb; ++q) {
            const unsigned long long f = ord[q];
            if ((unsigned)(f >> 32) != row) break;
            s += (double)__uint_as_float((unsigned)f);
        }
        p.vsum[bn + row] = s;
    }
    __syncthreads();  // ord[] goes to the row order next
}

// ------------------------------------------------------------------------------------------
// One workgroup per instance.  Dynamic LDS: ord[p2] 64-bit words (p2 = n rounded up to a power of two),
// then the used-column bitmap.  ord holds the sort keys (f32_key(m_i) << 32 | i), then per position of
// the row order (first column to try << 32 | row), then (column taken << 32 | row), and at the end the
// matched costs by row.
// ------------------------------------------------------------------------------------------
// kDual: the third term is v_reg of the DualGNN loss, and S_i and d_j are left for its backward.
template <bool kDual>
__global__ void __launch_bounds__(kTlGreedyThreads) tl_greedy_kernel(TrainLossParams p, int p2)
{
    extern __shared__ unsigned long long ord[];
    __shared__ BlockExchange ex;
    __shared__ int next_k;
    unsigned *used = reinterpret_cast<unsigned *>(ord + p2);
    const int b = blockIdx.x, n = p.n, tid = threadIdx.x, nt = blockDim.x;
    const int nb = tl_size(p.sizes[b], n);
    float *terms = p.terms + (size_t)b * kTlTerms;
    if (nb == 0) {
        if (tid == 0) {
            for (int t = 0; t < kTlTerms; ++t) terms[t] = f32_nan();
            p.ret[b] = kTrainLossBadSize;
        }
        return;
    }
    BlockCtx bc;
    bc.init(&ex);
    const size_t bn = (size_t)b * n;
    const float *Cb = p.C + bn * n;
    const float *ub = p.u + bn, *vb = p.v + bn;

    // integer scatters for the backward
    for (int j = tid; j < nb; j += nt) {
        const int a = p.arow[bn + j];
        if ((unsigned)a < (unsigned)nb) {
            atomicAdd(&p.cnt[bn + a], 1);
            const int kj = p.K[bn + j];
            if (kj) atomicAdd(&p.ksum[bn + a], kj);
        }
    }
    // the O(n) sums and the hinge partials
    double su = 0.0, sv = 0.0, sr = 0.0, sh = 0.0;
    for (int i = tid; i < nb; i += nt) {
        const float ui = ub[i];
        const float d = kDual ? p.vh[bn + i] - vb[i] : ui - p.ut[bn + i];
        const float q = d * d;
        su += (double)ui;
        sv += (double)vb[i];
        sr += (double)q;
    }
    for (int t = tid; t < p.hparts; t += nt) sh += p.hpart[(size_t)b * p.hparts + t];
    su = bc.sum_f64(su);
    sv = bc.sum_f64(sv);
    sr = bc.sum_f64(sr);
    sh = bc.sum_f64(sh);
    if constexpr (kDual) tl_segment_sums(p, ord, p2, bn, nb, tid, nt);

    // row order: ascending (m_i, i)
    for (int i = tid; i < p2; i += nt)
        ord[i] = (i < nb) ? (((unsigned long long)p.mkey[bn + i] << 32) | (unsigned)i) : ~0ull;
    for (int w = tid; w < (n + 31) / 32; w += nt) used[w] = 0u;
    __syncthreads();
    tl_bitonic_sort(ord, p2, tid, nt);
    for (int k = tid; k < nb; k += nt) {
        const unsigned row = (unsigned)ord[k];
        ord[k] = ((unsigned long long)(unsigned)p.mj[bn + row] << 32) | row;
    }
    __syncthreads();

    // Greedy.  A row whose own cheapest column is still free takes it without a scan: wave 0 runs such
    // rows back to back; at the first row that has to search, the whole workgroup scans it.
    int k = 0;
    for (;;) {
        if (bc.wave == 0) {
            while (k < nb) {
                const unsigned long long e = ord[k];
                const int j0 = uni((int)(unsigned)(e >> 32));
                if ((unsigned)j0 >= (unsigned)nb) break;
                const unsigned w = used[j0 >> 5];
                if ((w >> (j0 & 31)) & 1u) break;
                used[j0 >> 5] = w | (1u << (j0 & 31));  // every lane stores the same word
                ++k;
            }
            if (bc.lane == 0) next_k = k;
        }
        __syncthreads();
        k = next_k;
        if (k >= nb) break;
        const int row = (int)(unsigned)ord[k];
        const float ui = ub[row];
        const float *crow = Cb + (size_t)row * n;
        unsigned long long best = ~0ull;
        for (int j = tid; j < nb; j += nt) {
            if ((used[j >> 5] >> (j & 31)) & 1u) continue;
            const unsigned long long key = tl_pack((crow[j] - ui) - vb[j], j);
            best = (key < best) ? key : best;
        }
        best = bc.reduce<MinU64>(best);
        const int js = (int)(unsigned)best;  // some column is free: js < nb
        if (tid == 0) {
            used[js >> 5] |= 1u << (js & 31);
            ord[k] = ((unsigned long long)(unsigned)js << 32) | (unsigned)row;
        }
        ++k;
        __syncthreads();
    }

    // assignment out, matched costs by row into LDS, then their serial fp64 sum in row order
    int rows[kTlEpt];
    float cost[kTlEpt];
#pragma unroll
    for (int e = 0; e < kTlEpt; ++e) {
        const int q = tid + e * nt;
        rows[e] = -1;
        cost[e] = 0.0f;
        if (q < nb) {
            const unsigned long long w = ord[q];
            const int row = (int)(unsigned)w, col = (int)(unsigned)(w >> 32);
            rows[e] = row;
            cost[e] = Cb[(size_t)row * n + col];
            p.assign[bn + row] = col;
        }
    }
    __syncthreads();
    double *cval = reinterpret_cast<double *>(ord);
#pragma unroll
    for (int e = 0; e < kTlEpt; ++e)
        if (rows[e] >= 0) cval[rows[e]] = (double)cost[e];
    __syncthreads();
    if (tid == 0) {
        double pu = 0.0;
        for (int i = 0; i < nb; ++i) pu += cval[i];
        const double dn = (double)nb;
        terms[0] = (float)(su + sv);
        terms[1] = (float)(sh / (dn * dn));
        terms[2] = (float)(sr / dn);
        terms[3] = (float)pu;
        p.ret[b] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// Backward, one thread per (b, i):
//   g_i = grad_scale * [ w0 (cnt_i - 1) + w1 (R_i - sum_{a_j = i} K_j) / n_b^2 + w2 2 (u_i - t_i) / n_b ]
// in fp64, rounded once; 0 on padded rows.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTlThreads)
tl_backward_kernel(TrainLossParams p, const float *weights, float grad_scale, float *grad_u)
{
    const int b = blockIdx.y, n = p.n;
    const int i = blockIdx.x * kTlThreads + threadIdx.x;
    if (i >= n) return;
    const int nb = tl_size(p.sizes[b], n);
    const size_t o = (size_t)b * n + i;
    double g = 0.0;
    if (i < nb) {
        const double dn = (double)nb;
        const double gap = (double)(p.cnt[o] - 1);
        const double feas = (double)(p.R[o] - p.ksum[o]) / (dn * dn);
        const double reg = 2.0 * ((double)p.u[o] - (double)p.ut[o]) / dn;
        g = (double)grad_scale * ((double)weights[0] * gap + (double)weights[1] * feas + (double)weights[2] * reg);
    }
    grad_u[o] = (float)g;
}

// DualGNN backward, one thread per (b, i) and, with the same index, per (b, j):
//   grad_u_i  = grad_scale * [ w0 (cnt_i - 1) + w1 (R_i - sum_{a_j = i} K_j) / n_b^2 + w2 2 S_i / n_b ]
//   grad_vh_j = grad_scale * w2 2 d_j / n_b
// in fp64, rounded once; 0 on the padding.
__global__ void __launch_bounds__(kTlThreads)
tl_dual_backward_kernel(TrainLossParams p, const float *weights, float grad_scale, float *grad_u, float *grad_vh)
{
    const int b = blockIdx.y, n = p.n;
    const int i = blockIdx.x * kTlThreads + threadIdx.x;
    if (i >= n) return;
    const int nb = tl_size(p.sizes[b], n);
    const size_t o = (size_t)b * n + i;
    double g = 0.0, gv = 0.0;
    if (i < nb) {
        const double dn = (double)nb;
        const double gap = (double)(p.cnt[o] - 1);
        const double feas = (double)(p.R[o] - p.ksum[o]) / (dn * dn);
        const double reg = 2.0 * p.vsum[o] / dn;
        g = (double)grad_scale * ((double)weights[0] * gap + (double)weights[1] * feas + (double)weights[2] * reg);
        gv = (double)grad_scale * ((double)weights[2] * (2.0 * (double)p.dj[o] / dn));
    }
    grad_u[o] = (float)g;
    grad_vh[o] = (float)gv;
}

int tl_pow2(int n)
{
    int q = 1;
    while (q < n) q <<= 1;
    return q;
}

}  // namespace

void train_loss_plan(TrainLossParams *p)
{
    p->chunks = colmin_chunks(p->n, p->batch);
    // about 2048 workgroups of four waves for the hinge pass, at least one row per wave
    int rows = (int)(((size_t)p->n * p->batch + 2048 * kTlWaves - 1) / (2048 * kTlWaves));
    if (rows < 1) rows = 1;
    p->rows_per_wave = rows;
    const int blocks = (p->n + rows * kTlWaves - 1) / (rows * kTlWaves);
    p->hparts = blocks * kTlWaves;
}

hipError_t launch_train_loss_forward(const TrainLossParams &p, hipStream_t stream)
{
    const int n = p.n, batch = p.batch;
    const bool vec = (n % 4) == 0 && (reinterpret_cast<uintptr_t>(p.C) % 16) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.v) % 16) == 0;
    const int rows_per = (n + p.chunks - 1) / p.chunks;
    const int cols_per_block = kTlThreads * (vec ? 4 : 1);
    const dim3 g1((n + cols_per_block - 1) / cols_per_block, p.chunks, batch);
    hipLaunchKernelGGL(vec ? tl_colmin_partial_kernel<4> : tl_colmin_partial_kernel<1>, g1, dim3(kTlThreads), 0,
                       stream, p, rows_per);
    hipLaunchKernelGGL(tl_colmin_final_kernel, dim3((n + kTlThreads - 1) / kTlThreads, batch), dim3(kTlThreads), 0,
                       stream, p);
    hipLaunchKernelGGL(vec ? tl_hinge_kernel<4> : tl_hinge_kernel<1>, dim3(p.hparts / kTlWaves, batch),
                       dim3(kTlThreads), 0, stream, p);
    const int p2 = tl_pow2(n);
    const size_t lds = sizeof(unsigned long long) * (size_t)p2 + sizeof(unsigned) * (size_t)((n + 31) / 32);
    // always the limit of the largest n, never this call's size: calls from several host threads with
    // different n then cannot lower it under each other's launches
    constexpr int kMaxLds = (int)(sizeof(unsigned long long) * kTrainLossMaxN + sizeof(unsigned) * (kTrainLossMaxN / 32));
    const auto greedy = p.vh ? tl_greedy_kernel<true> : tl_greedy_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(greedy),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) return e;
    int threads = (n + kWave - 1) / kWave * kWave;
    if (threads > kTlGreedyThreads) threads = kTlGreedyThreads;
    hipLaunchKernelGGL(greedy, dim3(batch), dim3(threads), lds, stream, p, p2);
    return hipGetLastError();
}

hipError_t launch_train_loss_backward(const TrainLossParams &p, const float *weights, float grad_scale,
                                      float *grad_u, hipStream_t stream)
{
    hipLaunchKernelGGL(tl_backward_kernel, dim3((p.n + kTlThreads - 1) / kTlThreads, p.batch), dim3(kTlThreads), 0,
                       stream, p, weights, grad_scale, grad_u);
    return hipGetLastError();
}

hipError_t launch_dual_loss_backward(const TrainLossParams &p, const float *weights, float grad_scale, float *grad_u,
                                     float *grad_vh, hipStream_t stream)
{
    hipLaunchKernelGGL(tl_dual_backward_kernel, dim3((p.n + kTlThreads - 1) / kTlThreads, p.batch), dim3(kTlThreads),
                       0, stream, p, weights, grad_scale, grad_u, grad_vh);
    return hipGetLastError();
}

}  // namespace lapwarm
