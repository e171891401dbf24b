// oracle_duals.hip -- oracle dual reconstruction from a full matching, gfx950, fp64.
//
// Reference: solvers/dual_computation.py:13-74 `dual_from_matching_diff_constraints`.  For the
// pairs (r_k, a_k) the constraints are v_j <= v_a + fl(C[r,j] - C[r,a]); the reference solves
// them with Gauss-Seidel Bellman-Ford rounds from v = 0 (strict compare, one fp64 add).
//
// What runs here:
//   * frontier Jacobi sweeps, batched: v_new[j] = v_old[j] > cand_j ? cand_j : v_old[j] with
//     cand_j = min over the ACTIVE rows i of fl(v_old[x_i] + fl(C[i,j] - C[i,x_i])).  Row i is
//     active in a sweep iff v[x_i] changed in the previous one (all rows in the first): the rows
//     left out only repeat candidates v_old[j] already beats, so the fixed point and the sweep
//     count are those of full Jacobi sweeps.  v is double-buffered (Jacobi, not chaotic).
//     Jacobi and the reference's Gauss-Seidel converge to the same fixed point (the greatest one
//     <= 0 of a monotone operator), Gauss-Seidel in no more rounds; so when the Jacobi sweeps
//     settle after J <= n - 2 updating sweeps, the reference breaks out of its loop with exactly
//     this v.
//   * exact replay (one workgroup per instance) of the reference's Gauss-Seidel loop in the
//     caller's pair order, for the instances whose Jacobi sweeps do not settle within n - 1
//     sweeps or whose predecessor graph has a cycle (checked after every chunk of sweeps);
//     n <= kReplayMaxN.  Above that size a predecessor cycle is reported as the negative cycle
//     directly -- the only decision that is not replayed.
//   * finish: u from the matched pairs, the gauge shift with numpy's pairwise-sum order of
//     np.mean, the matched |reduced cost| maximum; the reduced-cost minimum is the dense
//     launch_reduced_min sweep ((C - u_i) - v_j, the reference's order).
//
// A ragged batch (ragged_batch.hpp) runs the same kernel bodies with a per-instance view: one init, one shared
// chain of sweeps, and each instance keeps the sweep budget and the check points it has alone.
#include "device_utils.hpp"
#include "dense_sweeps.hpp"  // colmin_chunks, launch_reduced_min
#include "oracle_duals.hpp"
#include "ragged_batch.hpp"

namespace lapwarm {

namespace {

constexpr int kOdThreads = 256;      // sweep kernels: 2 columns per lane
constexpr int kOdRowsPerChunk = 32;  // fewest active rows a partial block is given
constexpr int kReplayThreads = 1024;
constexpr int kReplayEpt = kOracleReplayMaxN / kReplayThreads;
constexpr int kCycleThreads = 1024;

__device__ __forceinline__ bool od_finite(double x) { return (x - x) == 0.0; }

// One body per kernel, two addressings.  Every per-instance array has the row stride p.n in both: that is n
// in a uniform batch and the padded width N in a ragged one, where instance b uses the prefix n_b of its row.
// Uniform: instance b is the n x n block at C + b * n * n, and the pair load is the host's choice for the
// whole batch.  RAGGED (ragged_batch.hpp): n_b x n_b at C + offsets[b] with row stride ld, or n_b when
// packed; the 16-byte pair load is taken when n_b and the row stride are even and the base is 16-byte
// aligned (offsets are multiples of 8 bytes only), decided here per instance, workgroup-uniform.
struct OdInstance {
    int n;
    size_t ld;        // row stride of C
    const double *C;
    bool pair;
};

template <bool RAGGED>
__device__ __forceinline__ OdInstance od_instance(const OracleParams &p, int b)
{
    OdInstance t;
    if constexpr (RAGGED) {
        const RaggedBatch g{p.C, p.offsets, p.sizes, p.ld, p.batch, p.n};
        t.n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
        t.ld = p.ld ? (size_t)p.ld : (size_t)t.n;
        t.C = p.C + p.offsets[b];
        t.pair = (t.n % 2) == 0 && (t.ld % 2) == 0 && (reinterpret_cast<uintptr_t>(t.C) % 16) == 0;
    } else {
        t.n = p.n;
        t.ld = (size_t)p.n;
        t.C = p.C + (size_t)b * p.n * p.n;
        t.pair = p.pair != 0;
    }
    return t;
}

// ------------------------------------------------------------------------------------------
// Set-up, one workgroup per instance: check that the pairs form a permutation, x (row -> col),
// y (col -> row), C[i][x_i], v = 0, no predecessors, every row active with source value 0.
// ------------------------------------------------------------------------------------------
// A ragged instance that is treated as empty (ragged_size) gets kOracleEmpty here and no kernel touches it again.
template <bool RAGGED>
__global__ void __launch_bounds__(kOdThreads) od_init_kernel(OracleParams p)
{
    const OdInstance t = od_instance<RAGGED>(p, blockIdx.x);
    const int b = blockIdx.x, n = t.n, tid = threadIdx.x;
    const size_t bn = (size_t)b * p.n;
    int *x = p.x + bn, *y = p.y + bn;
    for (int i = tid; i < n; i += kOdThreads) {
        x[i] = -1;
        y[i] = -1;
    }
    __syncthreads();
    int bad = 0;
    for (int k = tid; k < n; k += kOdThreads) {
        const int r = p.rows[bn + k], a = p.cols[bn + k];
        if (r < 0 || r >= n || a < 0 || a >= n) {
            bad = 1;
            continue;
        }
        if (atomicCAS(&x[r], -1, a) != -1) bad = 1;
        if (atomicCAS(&y[a], -1, r) != -1) bad = 1;
    }
    bad = __syncthreads_or(bad);
    int nonfinite = 0;
    if (!bad) {
        for (int i = tid; i < n; i += kOdThreads) {
            const double c = t.C[(size_t)i * t.ld + x[i]];
            nonfinite |= !od_finite(c);
            p.cxx[bn + i] = c;
            p.lrow[bn + i] = i;
            p.lsrc[bn + i] = 0.0;
            p.v0[bn + i] = 0.0;
            p.pred[bn + i] = -1;
        }
    }
    nonfinite = __syncthreads_or(nonfinite);
    if (tid == 0) {
        int *st = p.inst + (size_t)b * kOdInstInts;
        st[kOdStatus] = bad ? kOracleNotPermutation : (nonfinite ? kOracleNonFinite : 0);
        if (RAGGED && n == 0) st[kOdStatus] = kOracleEmpty;
        st[kOdCount0] = n;
        st[kOdCount1] = 0;
        st[kOdSweeps] = 0;
        st[kOdDepth] = 0;
        st[kOdRowsRead] = 0;
        st[kOdReplayed] = 0;
        st[kOdSlackBad] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// One frontier sweep, part 1: grid (column tiles, chunks, batch).  Chunk c takes an equal share
// of the active list (at least kOdRowsPerChunk entries), 2 columns per lane, and writes its
// column minima with the row that gave them (ties: the smallest row).  The first sweep reads
// every element of C and checks it is finite.  RAGGED: the sweep number is the batch's, the budget the
// instance's own -- an instance that has made its n_b - 1 sweeps is skipped, so at every check its state is
// what it is alone; blocks and lanes right of the prefix leave at once.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int od_chunks_used(int cnt, int chunks)
{
    int c = (cnt + kOdRowsPerChunk - 1) / kOdRowsPerChunk;
    return c < chunks ? c : chunks;
}

template <bool RAGGED>
__global__ void __launch_bounds__(kOdThreads) od_sweep_partial_kernel(OracleParams p, int s)
{
    const int b = blockIdx.z, chunk = blockIdx.y;
    int *st = p.inst + (size_t)b * kOdInstInts;
    const int cur = s & 1;
    const int cnt = st[kOdCount0 + cur];
    const OdInstance t = od_instance<RAGGED>(p, b);
    if (st[kOdStatus] != 0) return;
    const int n = t.n;
    if (RAGGED && s >= n - 1) return;
    if (cnt == 0) {
        if (blockIdx.x == 0 && chunk == 0 && threadIdx.x == 0) st[kOdStatus] = kOracleDone;
        return;
    }
    if (blockIdx.x == 0 && chunk == 0 && threadIdx.x == 0) st[kOdCount0 + (cur ^ 1)] = 0;
    const int used = od_chunks_used(cnt, p.chunks);
    if (chunk >= used) return;
    const int per = (cnt + used - 1) / used;
    const int q0 = chunk * per;
    const int q1 = (q0 + per < cnt) ? q0 + per : cnt;
    const int j = (blockIdx.x * kOdThreads + threadIdx.x) * 2;
    if (j >= n) return;
    const bool two = (j + 1) < n;
    const size_t bn = (size_t)b * p.n;
    const size_t lo = (size_t)cur * p.batch * p.n + bn;
    const int *lrow = p.lrow + lo;
    const double *lsrc = p.lsrc + lo;
    const double *Cb = t.C;
    double m0 = pos_inf(), m1 = pos_inf();
    int a0 = 0x7fffffff, a1 = 0x7fffffff;
    int nonfinite = 0;
    const bool first = (s == 0);
#pragma unroll 4
    for (int q = q0; q < q1; ++q) {
        const int i = lrow[q];
        const double src = lsrc[q];
        const double base = p.cxx[bn + i];
        const double *row = Cb + (size_t)i * t.ld + j;
        double c0, c1;
        if (t.pair) {
            const double2 c = *reinterpret_cast<const double2 *>(row);
            c0 = c.x;
            c1 = c.y;
        } else {
            c0 = row[0];
            c1 = two ? row[1] : 0.0;
        }
        if (first && !(od_finite(c0) && (!two || od_finite(c1)))) nonfinite = 1;
        const double t0 = src + (c0 - base);
        const double t1 = src + (c1 - base);
        if (t0 < m0 || (t0 == m0 && i < a0)) {
            m0 = t0;
            a0 = i;
        }
        if (t1 < m1 || (t1 == m1 && i < a1)) {
            m1 = t1;
            a1 = i;
        }
    }
    if (first && nonfinite) atomicCAS(&st[kOdStatus], 0, kOracleNonFinite);
    const size_t po = ((size_t)b * p.chunks + chunk) * p.n + j;
    p.pval[po] = m0;
    p.parg[po] = a0;
    if (two) {
        p.pval[po + 1] = m1;
        p.parg[po + 1] = a1;
    }
}

// Part 2: grid (column blocks, batch).  Combine the chunks, apply the strict update into the
// other v buffer, record the predecessor row, and append the row matched to every changed column
// (with its new source value) to the next active list.
template <bool RAGGED>
__global__ void __launch_bounds__(kOdThreads) od_sweep_final_kernel(OracleParams p, int s)
{
    const int b = blockIdx.y;
    int *st = p.inst + (size_t)b * kOdInstInts;
    const int cur = s & 1;
    const int cnt = st[kOdCount0 + cur];
    const int n = od_instance<RAGGED>(p, b).n;
    if (st[kOdStatus] != 0 || cnt == 0) return;
    if (RAGGED && s >= n - 1) return;
    const int j = blockIdx.x * kOdThreads + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kOdSweeps] = s + 1;
        st[kOdRowsRead] += cnt;
    }
    if (j >= n) return;
    const size_t bn = (size_t)b * p.n;
    const double *vo = (cur ? p.v1 : p.v0) + bn;
    double *vn = (cur ? p.v0 : p.v1) + bn;
    const int used = od_chunks_used(cnt, p.chunks);
    double m = pos_inf();
    int arg = 0x7fffffff;
    for (int c = 0; c < used; ++c) {
        const size_t po = ((size_t)b * p.chunks + c) * p.n + j;
        const double t = p.pval[po];
        const int a = p.parg[po];
        if (t < m || (t == m && a < arg)) {
            m = t;
            arg = a;
        }
    }
    const double old = vo[j];
    if (old > m) {
        vn[j] = m;
        p.pred[bn + j] = arg;
        const int i = p.y[bn + j];
        const int q = atomicAdd(&st[kOdCount0 + (cur ^ 1)], 1);
        const size_t lo = (size_t)(cur ^ 1) * p.batch * p.n + bn;
        p.lrow[lo + q] = i;
        p.lsrc[lo + q] = m;
        st[kOdDepth] = s + 1;  // every writer stores the same value
    } else {
        vn[j] = old;
    }
}

// ------------------------------------------------------------------------------------------
// After a chunk of sweeps, one workgroup per running instance: stop the converged ones, detect a
// cycle in the predecessor graph (column j -> column x[pred[j]]) by pointer doubling in LDS, and
// at the end of the sweep budget hand the unsettled ones to the replay.  `running` counts the
// instances that still need sweeps.  RAGGED: s is the batch's sweep number; the instance has made
// min(s, n_b - 1) sweeps -- that is the parity of its lists -- and its budget ends at s >= n_b - 1, or with the
// host's `last` (a device size above every host size: the schedule ends before the instance's own budget).
// ------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(kCycleThreads) od_check_kernel(OracleParams p, int s, int last, int *running)
{
    extern __shared__ int q[];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *st = p.inst + (size_t)b * kOdInstInts;
    const int n = od_instance<RAGGED>(p, b).n;
    if (st[kOdStatus] != 0) return;
    if constexpr (RAGGED) {  // the host's `last` still ends an instance whose budget lies beyond the host's
        if (s >= n - 1) {
            last = 1;
            s = n - 1;
        }
    }
    const int cnt = st[kOdCount0 + (s & 1)];
    if (cnt == 0) {
        if (tid == 0) st[kOdStatus] = kOracleDone;
        return;
    }
    const size_t bn = (size_t)b * p.n;
    for (int j = tid; j < n; j += kCycleThreads) {
        const int pr = p.pred[bn + j];
        q[j] = pr < 0 ? -1 : p.x[bn + pr];
    }
    __syncthreads();
    // 2^rounds >= 2n: a chain that reaches a root does so within n steps
    int rounds = 1;
    while ((1 << (rounds - 1)) < n) ++rounds;
    for (int r = 0; r < rounds; ++r) {
        int nxt[kOracleMaxN / kCycleThreads];
#pragma unroll
        for (int e = 0; e < kOracleMaxN / kCycleThreads; ++e) {
            const int j = tid + e * kCycleThreads;
            if (j < n) {
                const int t = q[j];
                nxt[e] = t < 0 ? -1 : q[t];
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kOracleMaxN / kCycleThreads; ++e) {
            const int j = tid + e * kCycleThreads;
            if (j < n) q[j] = nxt[e];
        }
        __syncthreads();
    }
    int cyc = 0;
    for (int j = tid; j < n; j += kCycleThreads) cyc |= (q[j] >= 0);
    cyc = __syncthreads_or(cyc);
    if (tid == 0) {
        if (cyc || last) {
            st[kOdStatus] = (n <= kOracleReplayMaxN) ? kOracleReplay : kOracleNegativeCycle;
        } else {
            atomicAdd(running, 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Exact replay of the reference's loop, one workgroup per instance flagged kOracleReplay:
// rounds of the pairs in the caller's order; within a pair the n edge updates are independent
// (only the self-edge, weight 0, touches v[a], and it never fires), so one pair is one
// workgroup-wide step.  Then the tol check of the `for ... else` clause.
// ------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(kReplayThreads) od_replay_kernel(OracleParams p, double tol)
{
    __shared__ double vl[kOracleReplayMaxN];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *st = p.inst + (size_t)b * kOdInstInts;
    if (st[kOdStatus] != kOracleReplay) return;
    const OdInstance inst = od_instance<RAGGED>(p, b);
    const int n = inst.n;
    const size_t ld = inst.ld;
    const size_t bn = (size_t)b * p.n;
    const double *Cb = inst.C;
    const int *rows = p.rows + bn, *cols = p.cols + bn;
    for (int j = tid; j < n; j += kReplayThreads) vl[j] = 0.0;
    __syncthreads();
    bool broke = false;
    for (int round = 0; round < n - 1; ++round) {
        int upd = 0;
        double c[kReplayEpt];
        {
            const double *row = Cb + (size_t)rows[0] * ld;
#pragma unroll
            for (int e = 0; e < kReplayEpt; ++e) {
                const int j = tid + e * kReplayThreads;
                c[e] = (j < n) ? row[j] : 0.0;
            }
        }
        for (int k = 0; k < n; ++k) {
            const int a = cols[k];
            const double base = Cb[(size_t)rows[k] * ld + a];
            const double va = vl[a];
            double cn[kReplayEpt];
            const double *nrow = Cb + (size_t)rows[(k + 1 < n) ? k + 1 : k] * ld;
#pragma unroll
            for (int e = 0; e < kReplayEpt; ++e) {
                const int j = tid + e * kReplayThreads;
                cn[e] = (j < n) ? nrow[j] : 0.0;
            }
#pragma unroll
            for (int e = 0; e < kReplayEpt; ++e) {
                const int j = tid + e * kReplayThreads;
                if (j < n) {
                    const double t = va + (c[e] - base);
                    if (vl[j] > t) {
                        vl[j] = t;
                        upd = 1;
                    }
                }
                c[e] = cn[e];
            }
            __syncthreads();
        }
        if (!__syncthreads_or(upd)) {
            broke = true;
            break;
        }
    }
    int neg = 0;
    if (!broke) {
        for (int k = 0; k < n; ++k) {
            const double *row = Cb + (size_t)rows[k] * ld;
            const int a = cols[k];
            const double base = row[a];
            const double va = vl[a];
            for (int j = tid; j < n; j += kReplayThreads)
                if (vl[j] > (va + (row[j] - base)) - tol) neg = 1;
        }
    }
    neg = __syncthreads_or(neg);
    const int sw = st[kOdSweeps];
    double *vout = ((sw & 1) ? p.v1 : p.v0) + bn;
    for (int j = tid; j < n; j += kReplayThreads) vout[j] = vl[j];
    if (tid == 0) {
        st[kOdReplayed] = 1;
        st[kOdStatus] = neg ? kOracleNegativeCycle : kOracleDone;
    }
}

// ------------------------------------------------------------------------------------------
// Finish, one workgroup per instance: u_r = C[r][x_r] - v[x_r]; shift = (mean(u) + mean(v)) / 2;
// u -= shift, v += shift; max over matched edges of |(C - u) - v|.  Instances that failed get NaN.
// RAGGED: all of this on the prefix n_b; u and v are 0 beyond it.
// ------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(kOdThreads) od_finish_kernel(OracleParams p, double *u_out, double *v_out)
{
    __shared__ double sh[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *st = p.inst + (size_t)b * kOdInstInts;
    const size_t bn = (size_t)b * p.n;
    double *u = u_out + bn, *v = v_out + bn;
    int n = p.n;
    if constexpr (RAGGED) {
        n = od_instance<true>(p, b).n;
        for (int j = n + tid; j < p.n; j += kOdThreads) {
            u[j] = 0.0;
            v[j] = 0.0;
        }
    }
    if (st[kOdStatus] != kOracleDone) {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int j = tid; j < n; j += kOdThreads) {
            u[j] = qnan;
            v[j] = qnan;
        }
        return;
    }
    const int sw = st[kOdSweeps];
    const double *vs = ((sw & 1) ? p.v1 : p.v0) + bn;
    const int *x = p.x + bn;
    for (int i = tid; i < n; i += kOdThreads) {
        v[i] = vs[i];
        u[i] = p.cxx[bn + i] - vs[x[i]];
    }
    __syncthreads();
    if (tid == 0) sh[0] = pairwise_sum<10>(u, n) / (double)n;
    if (tid == kWave) sh[1] = pairwise_sum<10>(v, n) / (double)n;
    __syncthreads();
    const double shift = (sh[0] + sh[1]) / 2.0;
    for (int i = tid; i < n; i += kOdThreads) {
        u[i] = u[i] - shift;
        v[i] = v[i] + shift;
    }
    __syncthreads();
    int slack = 0;
    for (int i = tid; i < n; i += kOdThreads) {
        const double r = (p.cxx[bn + i] - u[i]) - v[x[i]];
        if (fabs(r) > 1e-6) slack = 1;
    }
    slack = __syncthreads_or(slack);
    if (tid == 0) st[kOdSlackBad] = slack;
}

// ret[b] and the per-instance counters, in the reference's order of checks.
__global__ void od_verdict_kernel(OracleParams p, const double *gmin, int *ret, int *sweeps)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.batch) return;
    const int *st = p.inst + (size_t)b * kOdInstInts;
    int r = st[kOdStatus];
    if (r == kOracleDone) {
        r = kOracleOk;
        if (gmin[b] < -1e-8)
            r = kOracleInfeasible;
        else if (st[kOdSlackBad])
            r = kOracleSlackness;
    }
    ret[b] = r;
    if (sweeps) {
        int *o = sweeps + (size_t)b * 4;
        o[0] = st[kOdSweeps];
        o[1] = st[kOdDepth];
        o[2] = st[kOdRowsRead];
        o[3] = st[kOdReplayed];
    }
}

}  // namespace

int oracle_chunks(int n, int batch) { return colmin_chunks(n, batch); }

hipError_t launch_oracle_init(const OracleParams &p, hipStream_t stream)
{
    if (p.sizes)
        hipLaunchKernelGGL(od_init_kernel<true>, dim3(p.batch), dim3(kOdThreads), 0, stream, p);
    else
        hipLaunchKernelGGL(od_init_kernel<false>, dim3(p.batch), dim3(kOdThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_oracle_sweep(const OracleParams &p, int s, hipStream_t stream)
{
    const dim3 g1((p.n + 2 * kOdThreads - 1) / (2 * kOdThreads), p.chunks, p.batch);
    const dim3 g2((p.n + kOdThreads - 1) / kOdThreads, p.batch);
    if (p.sizes) {
        hipLaunchKernelGGL(od_sweep_partial_kernel<true>, g1, dim3(kOdThreads), 0, stream, p, s);
        hipLaunchKernelGGL(od_sweep_final_kernel<true>, g2, dim3(kOdThreads), 0, stream, p, s);
    } else {
        hipLaunchKernelGGL(od_sweep_partial_kernel<false>, g1, dim3(kOdThreads), 0, stream, p, s);
        hipLaunchKernelGGL(od_sweep_final_kernel<false>, g2, dim3(kOdThreads), 0, stream, p, s);
    }
    return hipGetLastError();
}

hipError_t launch_oracle_check(const OracleParams &p, int s, int last, int *running, hipStream_t stream)
{
    const size_t lds = sizeof(int) * (size_t)p.n;
    auto *kernel = p.sizes ? od_check_kernel<true> : od_check_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.batch), dim3(kCycleThreads), lds, stream, p, s, last, running);
    return hipGetLastError();
}

hipError_t launch_oracle_finish(const OracleParams &p, double tol, double *u, double *v, double *rowpart,
                                double *gmin, int *ret, int *sweeps, hipStream_t stream)
{
    hipError_t e;
    if (p.sizes) {  // the replay serves n_b <= kOracleReplayMaxN: the check kernel flags no other instance
        hipLaunchKernelGGL(od_replay_kernel<true>, dim3(p.batch), dim3(kReplayThreads), 0, stream, p, tol);
        hipLaunchKernelGGL(od_finish_kernel<true>, dim3(p.batch), dim3(kOdThreads), 0, stream, p, u, v);
        const RaggedBatch g{p.C, p.offsets, p.sizes, p.ld, p.batch, p.n};
        e = launch_reduced_min_ragged(g, u, v, rowpart, gmin, stream);
    } else {
        if (p.n <= kOracleReplayMaxN)
            hipLaunchKernelGGL(od_replay_kernel<false>, dim3(p.batch), dim3(kReplayThreads), 0, stream, p, tol);
        hipLaunchKernelGGL(od_finish_kernel<false>, dim3(p.batch), dim3(kOdThreads), 0, stream, p, u, v);
        e = launch_reduced_min(p.C, p.n, p.batch, u, v, rowpart, gmin, stream);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(od_verdict_kernel, dim3((p.batch + 255) / 256), dim3(256), 0, stream, p, gmin, ret, sweeps);
    return hipGetLastError();
}

}  // namespace lapwarm
