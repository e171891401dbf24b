// dense_sweeps.hip -- the HBM-streaming passes over C[batch][n][n] (fp64, row-major), gfx950.
//
// Each kernel reads C exactly once, coalesced along j (consecutive lanes -> consecutive
// columns), reduces through wave64 shuffles and LDS partials, and writes O(n) results.
// Reference behaviour reproduced (paths relative to /root/reference):
//   seeded prelude   LAP/_lapjv_cpp/lapjv_seeded.cpp:38-48 (candidate scan only), :9-17/:51-53
//                    (verify), :66-73 (row tightening), :76-93/:105-113 (tight-edge test/count)
//   projection       LAP/_lapjv_cpp/lapjv_seeded.cpp:38-48 (exact Gauss-Seidel replay)
//   min-trick        scripts/gnn_benchmark.py:262 ; column minima gnn/features.py:218
//   dual utilities   solvers/advanced_dual.py:14-63
//   row features     gnn/features.py:161-243
#include "device_utils.hpp"
#include "dense_sweeps.hpp"
#include "jv_solver.hpp"
#include "ragged_batch.hpp"

namespace lapwarm {

namespace {

constexpr int kSweepThreads = 256;

// ------------------------------------------------------------------------------------------
// Seeded prelude: one workgroup per row.  Fuses four of the reference's five O(n^2) loops:
// projection-candidate count, verify, row tightening, tight-edge bitmap + count.
// ------------------------------------------------------------------------------------------
// EPT > 0: the row (and v) stay in registers between the two passes (n <= EPT * kSweepThreads), so C
// is read from HBM exactly once; EPT == 0: rows of any length, second pass re-reads (L2).
// One body, two entries.  prelude_kernel: row i of instance b of a uniform batch.  RAGGED (prelude_ragged_kernel,
// ragged_batch.hpp): workgroup (i, b) owns row i of the padded [N] rows of instance b and leaves at once beyond
// n_b (workgroup-uniform: blockIdx and sizes[b] only); n_b is loaded once into a scalar; p.n is N, the stride of
// every [batch][.] array, and the bitmap of instance b is its n_b rows of ceil(n_b / 32) words, back to back, at
// b * N * ceil(N / 32) -- the layout the solver reads for an instance of that size alone.
template <int EPT, bool RAGGED>
__device__ __forceinline__ void prelude_body(const PreludeParams &p, const RaggedBatch &g)
{
    __shared__ BlockExchange ex;
    __shared__ uint32_t bits[512];  // n <= 16384
    const int b = blockIdx.y, i = blockIdx.x;
    int n_b = p.n;
    if constexpr (RAGGED) {
        n_b = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
        if (i >= n_b) return;
    }
    const int n = n_b;
    if (p.rerun && !(p.inst_flags[b] & kFlagProjected)) return;
    BlockCtx bc;
    bc.init(&ex);
    const int W = (n + 31) >> 5;
    for (int w = bc.tid; w < W; w += kSweepThreads) bits[w] = 0;

    const size_t rowoff = ((size_t)b * n + i) * n;
    const double *row = RAGGED ? g.C + g.offsets[b] + (size_t)i * (g.ld ? g.ld : n) : p.C + rowoff;
    const int pn = p.n;  // stride of the [batch][.] arrays: n, or N
    const double *vb = p.v + (size_t)b * pn;
    const double ui = p.u[(size_t)b * pn + i];
    const double eps = p.eps;
    const bool first = !p.rerun;

    constexpr int R = EPT > 0 ? EPT : 1;
    double c[R], vv[R];
    double m = pos_inf();
    int counts = 0;  // low 16 bits: projection candidates, high bits: verify failures
    if constexpr (EPT > 0) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int j = bc.tid + k * kSweepThreads;
            c[k] = (j < n) ? row[j] : pos_inf();
            vv[k] = (j < n) ? vb[j] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int j = bc.tid + k * kSweepThreads;
            if (j < n) {
                if (first && ((ui + vv[k]) - c[k]) > eps) counts += 1;
                if (((c[k] - ui) - vv[k]) < -eps) counts += 1 << 16;
                m = dmin(m, c[k] - vv[k]);
            }
        }
    } else {
        for (int j = bc.tid; j < n; j += kSweepThreads) {
            const double cj = row[j];
            const double vj = vb[j];
            if (first && ((ui + vj) - cj) > eps) counts += 1;
            if (((cj - ui) - vj) < -eps) counts += 1 << 16;
            m = dmin(m, cj - vj);
        }
    }
    m = bc.min_f64(m);
    counts = bc.sum_i32(counts);
    const double u_new = m;
    const double teps = p.tight_eps;
    if constexpr (EPT > 0) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int j = bc.tid + k * kSweepThreads;
            if (j < n && fabs((c[k] - u_new) - vv[k]) <= teps) atomicOr(&bits[j >> 5], 1u << (j & 31));
        }
    } else {
        for (int j = bc.tid; j < n; j += kSweepThreads) {
            const double r = (row[j] - u_new) - vb[j];
            if (fabs(r) <= teps) atomicOr(&bits[j >> 5], 1u << (j & 31));
        }
    }
    __syncthreads();
    int cnt = 0;
    uint32_t *out_bits = RAGGED ? p.tight_bits + (size_t)b * pn * ((pn + 31) >> 5) + (size_t)i * W
                                : p.tight_bits + ((size_t)b * n + i) * W;
    for (int w = bc.tid; w < W; w += kSweepThreads) {
        const uint32_t word = bits[w];
        out_bits[w] = word;
        cnt += __popc(word);
    }
    cnt = bc.sum_i32(cnt);
    if (bc.tid == 0) {
        const size_t o = (size_t)b * pn + i;
        p.u_tight[o] = u_new;
        p.tight_cnt[o] = cnt;
        const int viol = counts & 0xffff, bad = counts >> 16;
        int f = 0;
        if (first) {
            p.viol_cnt[o] = viol;
            if (viol > 0) f |= kFlagHasViolation;
        }
        if (bad > 0) f |= kFlagInfeasible;
        if (f) atomicOr(&p.inst_flags[b], f);
    }
}

template <int EPT>
__global__ void __launch_bounds__(kSweepThreads) prelude_kernel(PreludeParams p)
{
    prelude_body<EPT, false>(p, RaggedBatch{});
}

template <int EPT>
__global__ void __launch_bounds__(kSweepThreads) prelude_ragged_kernel(PreludeParams p, RaggedBatch g)
{
    prelude_body<EPT, true>(p, g);
}

// ------------------------------------------------------------------------------------------
// Projection (slow path, one workgroup per flagged instance).  u and v only ever decrease, and
// fl(fl(u+v)-C) is monotone in both, so an entry that is not a candidate under the seed duals
// can never fire: rows without candidates are skipped, the others replay the serial scan as
// "find the next firing column given the current u_i" with a workgroup-wide first-index search.
// ------------------------------------------------------------------------------------------
// The body: row i of the instance is Cb + (row0 + i) * ldc; ub / vb / vc are its n duals and candidate counts.
__device__ __forceinline__ void project_instance(BlockExchange *ex, const double *Cb, size_t row0, size_t ldc, int n,
                                                 double *ub, double *vb, const int *vc, int *inst_flags, int b,
                                                 int flags, double eps)
{
    BlockCtx bc;
    bc.init(ex);
    for (int i = 0; i < n; ++i) {
        if (vc[i] == 0) continue;
        const double *row = Cb + (row0 + i) * ldc;
        double ui = ub[i];
        int jstart = 0;
        for (int guard = 0; guard <= n; ++guard) {
            int cand = 0x7fffffff;
            for (int j = jstart + bc.tid; j < n; j += kSweepThreads) {
                if (((ui + vb[j]) - row[j]) > eps) {
                    cand = j;
                    break;
                }
            }
            cand = bc.min_i32(cand);
            if (cand == 0x7fffffff) break;
            const double viol = (ui + vb[cand]) - row[cand];
            const double adj = viol / 2.0;
            ui -= adj;
            __syncthreads();  // every thread has read vb[cand]
            if (bc.tid == 0) vb[cand] -= adj;
            __syncthreads();
            jstart = cand + 1;
        }
        if (bc.tid == 0) ub[i] = ui;
    }
    if (bc.tid == 0) inst_flags[b] = (flags | kFlagProjected) & ~kFlagInfeasible;
}

__global__ void __launch_bounds__(kSweepThreads)
projection_kernel(const double *C, int n, double *u, double *v, const int *viol_cnt,
                  int *inst_flags, double eps)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.x;
    const int flags = inst_flags[b];
    if (!(flags & kFlagHasViolation)) return;
    const size_t ob = (size_t)b * n;
    project_instance(&ex, C, ob, n, n, u + ob, v + ob, viol_cnt + ob, inst_flags, b, flags, eps);
}

// Ragged batch: u, v, viol_cnt [batch][N]; the matrix of instance b from its offset and size.
__global__ void __launch_bounds__(kSweepThreads)
projection_ragged_kernel(RaggedBatch g, double *u, double *v, const int *viol_cnt, int *inst_flags, double eps)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(ragged_size(g, b));
    if (n == 0) return;
    const int flags = inst_flags[b];
    if (!(flags & kFlagHasViolation)) return;
    const size_t ob = (size_t)b * g.N;
    project_instance(&ex, g.C + g.offsets[b], 0, g.ld ? g.ld : n, n, u + ob, v + ob, viol_cnt + ob, inst_flags, b,
                     flags, eps);
}

// ------------------------------------------------------------------------------------------
// Column minima: out[b][j] = min_i (C[b][i][j] - u[b][i]), NaN if any operand is (np.min).
// Two columns per lane (16 B loads)
// when n is even, a chunk of rows per workgroup, partial minima combined by a second kernel.
// ------------------------------------------------------------------------------------------
template <bool HAS_U, bool PAIR>
__global__ void __launch_bounds__(kSweepThreads)
colmin_partial_kernel(const double *C, int n, const double *u, double *partial, int rows_per, int chunks)
{
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int j = (blockIdx.x * kSweepThreads + threadIdx.x) * (PAIR ? 2 : 1);
    if (j >= n) return;
    const int i0 = chunk * rows_per;
    const int i1 = (i0 + rows_per < n) ? i0 + rows_per : n;
    const double *base = C + (size_t)b * n * n + j;
    const double *ub = HAS_U ? u + (size_t)b * n : nullptr;
    double m0 = pos_inf(), m1 = pos_inf();
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const double ui = HAS_U ? ub[i] : 0.0;
        if constexpr (PAIR) {
            const double2 c = *reinterpret_cast<const double2 *>(base + (size_t)i * n);
            m0 = nmin(m0, HAS_U ? c.x - ui : c.x);
            m1 = nmin(m1, HAS_U ? c.y - ui : c.y);
        } else {
            const double c = base[(size_t)i * n];
            m0 = nmin(m0, HAS_U ? c - ui : c);
        }
    }
    double *out = partial + ((size_t)b * chunks + chunk) * n + j;
    out[0] = m0;
    if constexpr (PAIR) out[1] = m1;
}

// mode 0: out = min over chunks ; mode 1: out = min(out, min over chunks)
__global__ void colmin_final_kernel(const double *partial, int n, int chunks, double *out, int mode)
{
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double m = mode ? out[(size_t)b * n + j] : pos_inf();
    for (int c = 0; c < chunks; ++c) m = nmin(m, partial[((size_t)b * chunks + c) * n + j]);
    out[(size_t)b * n + j] = m;
}

// ------------------------------------------------------------------------------------------
// Row-wise reductions: one workgroup per row.
//   kind 0: out[b][i]  = min_j (C - v_j)                 (v may be null)
//   kind 1: out[b][i]  = min(out[b][i], min_j (C - v_j)) (project_feasible's u cap)
//   kind 2: out[b][i]  = min_j ((C - u_i) - v_j)         (row part of the global reduced min)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSweepThreads)
rowmin_kernel(const double *C, int n, const double *u, const double *v, double *out, int kind)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.y, i = blockIdx.x;
    BlockCtx bc;
    bc.init(&ex);
    const double *row = C + ((size_t)b * n + i) * n;
    const double *vb = v ? v + (size_t)b * n : nullptr;
    const double ui = (kind == 2) ? u[(size_t)b * n + i] : 0.0;
    double m = pos_inf();
    for (int j = bc.tid; j < n; j += kSweepThreads) {
        const double c = row[j];
        double r;
        if (kind == 2)
            r = (c - ui) - vb[j];
        else
            r = vb ? c - vb[j] : c;
        m = nmin(m, r);
    }
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) {
        const size_t o = (size_t)b * n + i;
        out[o] = (kind == 1) ? nmin(out[o], m) : m;
    }
}

__global__ void __launch_bounds__(kSweepThreads) vecmin_kernel(const double *in, int n, double *out)
{
    __shared__ BlockExchange ex;
    const int b = blockIdx.x;
    BlockCtx bc;
    bc.init(&ex);
    double m = pos_inf();
    for (int j = bc.tid; j < n; j += kSweepThreads) m = nmin(m, in[(size_t)b * n + j]);
    m = bc.min_f64<NanMinF64>(m);
    if (bc.tid == 0) out[b] = m;
}

// out = (C - u_i) - v_j, optionally minus min(out) when that is negative (advanced_dual.py:47-53)
__global__ void __launch_bounds__(kSweepThreads)
reduce_costs_kernel(const double *C, int n, const double *u, const double *v, const double *gmin,
                    int shift_nonneg, double *out)
{
    const int b = blockIdx.y, i = blockIdx.x;
    const size_t off = ((size_t)b * n + i) * n;
    const double ui = u[(size_t)b * n + i];
    const double *vb = v + (size_t)b * n;
    const double g = gmin[b];
    const bool shift = shift_nonneg && (g < 0);
    for (int j = threadIdx.x; j < n; j += kSweepThreads) {
        double r = (C[off + j] - ui) - vb[j];
        if (shift) r = r - g;
        out[off + j] = r;
    }
}

// ------------------------------------------------------------------------------------------
// Row features: one workgroup per row, the row staged in LDS.
//
// The reference sorts every row twice (gnn/features.py:190 for the k smallest and the median,
// :199 for the median absolute deviation).  Only five order statistics of each sorted array are
// ever read -- the 16 smallest, the two middle elements -- so this kernel SELECTS them exactly
// instead of sorting: one 256-bucket histogram over a monotone map of the value
// (bucket = trunc((x - lo) * 255 / (hi - lo))), a workgroup prefix sum to find the bucket that
// holds each wanted rank, a gather of that bucket's (<= 64) members and a rank-by-counting in one
// wave.  Buckets that hold more than 64 members (ties, heavily skewed rows) are narrowed by 8-bit
// radix passes over the IEEE order key, or recognised as all-equal by a min/max reduction.  Every
// map used is monotone non-decreasing in x, so the selected values are the ones a sort would put
// at those ranks, bit for bit.
// ------------------------------------------------------------------------------------------
constexpr double kFeatEps = 1e-9;  // gnn/features.py:18
constexpr int kSelList = 64;       // bucket size one wave ranks directly

struct SelectState {
    unsigned hist[256];
    int wtot[2][4];
    int bin[3], kk[3], cnt[3], base[3], shift[3], lcount[3];
    unsigned long long prefix[3];
    int lowcount;
    double val[3];
    double list[2][kSelList];    // bucket members of targets 1, 2
    double comb[16 + kSelList];  // target 0: the (< 16) values below its bucket, then its bucket
    double top[16];
};
// followed in LDS by one byte per element: its first-level bucket

__device__ __forceinline__ unsigned long long order_key(double x)
{
    const long long bts = __double_as_longlong(x + 0.0);  // -0.0 -> +0.0
    return bts < 0 ? ~(unsigned long long)bts : ((unsigned long long)bts | 0x8000000000000000ull);
}

__device__ __forceinline__ int lin_bucket(double x, double lo, double scale)
{
    const double t = (x - lo) * scale;
    const int bk = (t >= 255.0) ? 255 : (int)t;
    return (t > 0.0) ? bk : 0;
}

// exclusive prefix sum of one int per thread over the 256-thread workgroup; one barrier
__device__ __forceinline__ int block_excl_scan(int c, const BlockCtx &bc, SelectState *st, int &par)
{
    int incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(incl, off, kWave);
        if (bc.lane >= off) incl += o;
    }
    const int p = par;
    par ^= 1;
    if (bc.lane == kWave - 1) st->wtot[p][bc.wave] = incl;
    __syncthreads();
    int add = 0;
    for (int w = 0; w < bc.wave; ++w) add += st->wtot[p][w];
    return incl - c + add;
}

// Exact order statistics rank[0..NT) (ascending ranks) of s[0..n), all values in [lo, hi].
// TOP: additionally the rank[0]+1 smallest values, ascending, into st->top (rank[0] <= 15).
// Results in out[]; every thread returns the same values.  Ends with a barrier.
template <int NT, bool TOP>
__device__ __forceinline__ void select_ranks(SelectState *st, const double *s, int n, double lo, double hi,
                                             const int (&rank)[NT], double (&out)[NT], BlockCtx &bc, int &par)
{
    const int tid = bc.tid;
    unsigned char *bucket_of = reinterpret_cast<unsigned char *>(st + 1);
    const double width = hi - lo;
    const double scale = (width > 0.0 && width < pos_inf()) ? 255.0 / width : 0.0;
    st->hist[tid] = 0;
    if (tid < NT) {
        st->lcount[tid] = 0;
        st->shift[tid] = 64;
        st->prefix[tid] = 0;
    }
    if (tid == 0) st->lowcount = 0;
    __syncthreads();
#pragma unroll 4
    for (int j = tid; j < n; j += kSweepThreads) {
        const int lb = lin_bucket(s[j], lo, scale);
        bucket_of[j] = (unsigned char)lb;
        atomicAdd(&st->hist[lb], 1u);
    }
    __syncthreads();
    {
        const int c = (int)st->hist[tid];
        const int excl = block_excl_scan(c, bc, st, par);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (excl <= rank[t] && rank[t] < excl + c) {
                st->bin[t] = tid;
                st->kk[t] = rank[t] - excl;
                st->cnt[t] = c;
                st->base[t] = excl;
            }
        }
    }
    __syncthreads();
    bool alleq[NT];
    double eqval[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        alleq[t] = false;
        eqval[t] = 0.0;
        bool first = true;
        while (st->cnt[t] > kSelList) {  // LDS value, rewritten only between barriers: uniform
            const int bin = st->bin[t], shift = st->shift[t];
            const unsigned long long prefix = st->prefix[t];
            const int kkt = st->kk[t];
            if (first || shift == 0) {
                first = false;
                double mn = pos_inf(), mx = -pos_inf();
                for (int j = tid; j < n; j += kSweepThreads) {
                    if (bucket_of[j] != bin) continue;
                    const double x = s[j];
                    if (shift == 64 || (order_key(x) >> shift) == prefix) {
                        mn = dmin(mn, x);
                        mx = (x > mx) ? x : mx;
                    }
                }
                mn = bc.min_f64(mn);
                mx = bc.max_f64(mx);
                if (mn == mx || shift == 0) {
                    alleq[t] = true;
                    eqval[t] = mn;
                    break;
                }
            }
            st->hist[tid] = 0;
            __syncthreads();
            for (int j = tid; j < n; j += kSweepThreads) {
                if (bucket_of[j] != bin) continue;
                const unsigned long long key = order_key(s[j]);
                if (shift == 64 || (key >> shift) == prefix)
                    atomicAdd(&st->hist[(unsigned)(key >> (shift - 8)) & 255u], 1u);
            }
            __syncthreads();
            const int c = (int)st->hist[tid];
            const int excl = block_excl_scan(c, bc, st, par);
            if (excl <= kkt && kkt < excl + c) {
                st->prefix[t] = (prefix << 8) | (unsigned long long)tid;
                st->shift[t] = shift - 8;
                st->kk[t] = kkt - excl;
                st->cnt[t] = c;
                st->base[t] += excl;
            }
            __syncthreads();
        }
    }
    // gather the members of each target's bucket (and, for TOP, everything below target 0's)
    {
        int bin[NT], shift[NT];
        unsigned long long prefix[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            bin[t] = st->bin[t];
            shift[t] = st->shift[t];
            prefix[t] = st->prefix[t];
        }
        const int off0 = TOP ? st->base[0] : 0;
        bool narrowed = false;  // some target went through radix passes: its members need the key
#pragma unroll
        for (int t = 0; t < NT; ++t) narrowed = narrowed || shift[t] != 64;
#pragma unroll 2
        for (int j = tid; j < n; j += kSweepThreads) {
            const int lb = bucket_of[j];
            bool any = false;
#pragma unroll
            for (int t = 0; t < NT; ++t) any = any || lb == bin[t];
            if (!(any || (TOP && lb < bin[0]))) continue;
            const double x = s[j];
            const unsigned long long key = narrowed ? order_key(x) : 0ull;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const unsigned long long hi_bits = (shift[t] == 64) ? 0ull : (key >> shift[t]);
                const bool same = lb == bin[t] && (shift[t] == 64 || hi_bits == prefix[t]);
                if (same && !alleq[t]) {
                    const int q = atomicAdd(&st->lcount[t], 1);
                    if (t == 0)
                        st->comb[off0 + q] = x;
                    else
                        st->list[t - 1][q] = x;
                }
                if (TOP && t == 0) {
                    const bool below = lb < bin[0] || (lb == bin[0] && shift[0] != 64 && hi_bits < prefix[0]);
                    if (below) st->comb[atomicAdd(&st->lowcount, 1)] = x;
                }
            }
        }
    }
    __syncthreads();
    // wave t ranks the bucket of target t by counting; wave 3 orders the smallest values
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (bc.wave == t && !alleq[t]) {
            const int cnt = st->cnt[t], kkt = st->kk[t];
            const double *L = (t == 0) ? st->comb + (TOP ? st->base[0] : 0) : st->list[t - 1];
            const double a = (bc.lane < cnt) ? L[bc.lane] : pos_inf();
            int r = 0;
            for (int q = 0; q < cnt; ++q) {
                const double o = L[q];
                r += (o < a || (o == a && q < bc.lane)) ? 1 : 0;
            }
            if (bc.lane < cnt && r == kkt) st->val[t] = a;
        }
    }
    if (TOP && bc.wave == 3) {
        const int base0 = st->base[0];
        const int m = base0 + (alleq[0] ? 0 : st->cnt[0]);
        const int l0 = bc.lane, l1 = bc.lane + kWave;
        const double a0 = (l0 < m) ? st->comb[l0] : pos_inf();
        const double a1 = (l1 < m) ? st->comb[l1] : pos_inf();
        int r0 = 0, r1 = 0;
        for (int q = 0; q < m; ++q) {
            const double o = st->comb[q];
            r0 += (o < a0 || (o == a0 && q < l0)) ? 1 : 0;
            r1 += (o < a1 || (o == a1 && q < l1)) ? 1 : 0;
        }
        if (l0 < m && r0 <= rank[0]) st->top[r0] = a0;
        if (l1 < m && r1 <= rank[0]) st->top[r1] = a1;
        if (alleq[0] && l0 >= base0 && l0 <= rank[0]) st->top[l0] = eqval[0];
        if (l0 > rank[0] && l0 < 16) st->top[l0] = pos_inf();
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) out[t] = alleq[t] ? eqval[t] : st->val[t];
}

// Three workgroup reductions behind one barrier: min(a), max(b), sum(c) (sum: butterfly inside a
// wave, then waves in index order -- the same association as BlockCtx::sum_f64).
__device__ __forceinline__ void reduce_min_max_sum(BlockCtx &bc, double &a, double &b, double &c)
{
    a = wave_min(a);
    b = wave_max(b);
    c = wave_sum_f64(c);
    const int p = bc.parity;
    bc.parity ^= 1;
    if (bc.lane == 0) {
        bc.ex->d[p][bc.wave] = a;
        bc.ex->d[p][kMaxWaves + bc.wave] = b;
        bc.ex->d[p][2 * kMaxWaves + bc.wave] = c;
    }
    __syncthreads();
    a = bc.ex->d[p][0];
    b = bc.ex->d[p][kMaxWaves];
    c = bc.ex->d[p][2 * kMaxWaves];
    for (int w = 1; w < bc.nwaves; ++w) {
        a = dmin(a, bc.ex->d[p][w]);
        const double o = bc.ex->d[p][kMaxWaves + w];
        b = (o > b) ? o : b;
        c += bc.ex->d[p][2 * kMaxWaves + w];
    }
}

// sum(a), sum(b), sum(c) (doubles) and sum(k1), sum(k2) (ints) behind one barrier
__device__ __forceinline__ void reduce_sum3_isum2(BlockCtx &bc, double &a, double &b, double &c, int &k1, int &k2)
{
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    c = wave_sum_f64(c);
    k1 = wave_sum_i32(k1);
    k2 = wave_sum_i32(k2);
    const int p = bc.parity;
    bc.parity ^= 1;
    if (bc.lane == 0) {
        bc.ex->d[p][bc.wave] = a;
        bc.ex->d[p][kMaxWaves + bc.wave] = b;
        bc.ex->d[p][2 * kMaxWaves + bc.wave] = c;
        bc.ex->i[p][bc.wave] = k1;
        bc.ex->i[p][kMaxWaves + bc.wave] = k2;
    }
    __syncthreads();
    a = bc.ex->d[p][0];
    b = bc.ex->d[p][kMaxWaves];
    c = bc.ex->d[p][2 * kMaxWaves];
    k1 = bc.ex->i[p][0];
    k2 = bc.ex->i[p][kMaxWaves];
    for (int w = 1; w < bc.nwaves; ++w) {
        a += bc.ex->d[p][w];
        b += bc.ex->d[p][kMaxWaves + w];
        c += bc.ex->d[p][2 * kMaxWaves + w];
        k1 += bc.ex->i[p][w];
        k2 += bc.ex->i[p][kMaxWaves + w];
    }
}

// What one workgroup gets for one row of an n x n instance.
struct FeatureRow {
    const double *row;  // its n costs
    const double *cm;   // the n column minima of its instance
    const float *pos;   // its 8 positional encodings
    float *feat;        // 21
    float *topk;        // 16, or null
    float *cost32;      // CAST: n floats, (float)row, or null
    int n;
};

// The row body of both feature kernels: the uniform batch (row_features_kernel) and the ragged one
// (row_features_ragged_kernel) differ only in where a row and its outputs are.  `npad` doubles of LDS are
// staged (npad >= n, even); CAST also writes the row as float32 while it is in registers on its way to LDS.
template <bool CAST>
__device__ __forceinline__ void row_features_body(const FeatureRow &r, int npad)
{
    extern __shared__ __align__(16) unsigned char smem[];
    BlockExchange *ex = reinterpret_cast<BlockExchange *>(smem);
    double *s = reinterpret_cast<double *>(smem + sizeof(BlockExchange));
    SelectState *st = reinterpret_cast<SelectState *>(s + npad);
    const int n = r.n;
    BlockCtx bc;
    bc.init(ex);
    int par = 0;
    const double *row = r.row;
    const double *cm = r.cm;

    double lo = pos_inf(), hi = -pos_inf(), sum = 0.0;
#pragma unroll 4
    for (int j = bc.tid; j < n; j += kSweepThreads) {
        const double x = row[j];
        lo = dmin(lo, x);
        hi = (x > hi) ? x : hi;
        sum += x;
        s[j] = x;
        if constexpr (CAST) {
            if (r.cost32) r.cost32[j] = (float)x;
        }
    }
    reduce_min_max_sum(bc, lo, hi, sum);
    const double mean = sum / n;
    const double thresh = lo * 1.1;

    // Entropy  -sum p log(p + eps),  p = e / (S + eps),  e = exp(-(x - lo))  (gnn/features.py:178-181).
    // When every element has either e == 0 (its term is exactly 0) or e >= 1e-6 n (so p >= 1e-6 and
    // eps / p <= 1e-3), log(p + eps) = log p + log1p(eps / p) = -(x - lo) - log D + eps / p - ..., and
    // the sum closes from three accumulators of THIS pass:
    //     entropy = T / D + (S / D) log D - m eps,   T = sum e (x - lo),  m = #{e > 0},
    // the dropped terms being <= (eps^2 / 2) sum 1/p <= 1e-9.  One log per row instead of one per
    // element; rows with a mid-range element (0 < e < 1e-6 n: wide cost ranges, e.g. the metric
    // family) take the element-wise pass below.  The decision is uniform over the row.
    double sq = 0.0, esum = 0.0, tsum = 0.0;
    int cnts = 0;  // low 16: near-best, high: column-best
    int mcnt = 0;  // low 20 bits: elements with e > 0; bits 20+: threads that saw an element with 0 < e < tau
    bool mid = false;
    const double tau = 1e-6 * (double)n;
#pragma unroll 2
    for (int j = bc.tid; j < n; j += kSweepThreads) {
        const double x = s[j];
        const double dlt = x - mean;
        sq += dlt * dlt;
        const double xl = x - lo;
        const double e = exp(-xl);
        esum += e;
        if (e > 0.0) {
            tsum += e * xl;
            mcnt += 1;
            mid = mid || (e < tau);
        }
        if (x <= thresh) cnts += 1;
        if (x == cm[j]) cnts += 1 << 16;
    }
    if (mid) mcnt += 1 << 20;  // at most once per thread: 256 << 20 fits an int
    reduce_sum3_isum2(bc, sq, esum, tsum, cnts, mcnt);
    const double denom = esum + kFeatEps;
    double ent;
    if ((mcnt >> 20) == 0) {
        ent = tsum / denom + (esum / denom) * log(denom) - (double)(mcnt & 0xfffff) * kFeatEps;
    } else {
        const double rdenom = 1.0 / denom;  // p = e * (1/denom): within one ulp of the quotient, far below float32
        ent = 0.0;
#pragma unroll 2
        for (int j = bc.tid; j < n; j += kSweepThreads) {
            const double e = exp(-(s[j] - lo));
            const double pj = e * rdenom;
            ent += pj * log(pj + kFeatEps);
        }
        ent = -bc.sum_f64(ent);
    }

    // order statistics of the row: the 16 smallest, the two middle elements
    const int rk[3] = {(n < 16 ? n : 16) - 1, (n - 1) >> 1, n >> 1};
    double sel[3];
    select_ranks<3, true>(st, s, n, lo, hi, rk, sel, bc, par);
    const double med = (n & 1) ? sel[2] : (sel[1] + sel[2]) / 2.0;
    const int kk = (n < 10) ? n : 10;
    double gap = 0.0, kmean = 0.0, kstd = 0.0;
    if (bc.tid == 0) {
        if (n >= 2) gap = st->top[1] - st->top[0];
        double acc = 0.0;
        for (int q = 0; q < kk; ++q) acc += st->top[q];
        kmean = acc / kk;
        double a2 = 0.0;
        for (int q = 0; q < kk; ++q) {
            const double dq = st->top[q] - kmean;
            a2 += dq * dq;
        }
        kstd = sqrt(a2 / kk);
        if (r.topk) {
            for (int q = 0; q < 16; ++q) r.topk[q] = (float)st->top[q];  // +inf beyond n
        }
    }
    // median absolute deviation: the same selection on |x - median|, which lies in [0, dmax]
    for (int j = bc.tid; j < n; j += kSweepThreads) s[j] = fabs(s[j] - med);
    const double dlo = fabs(lo - med), dhi = fabs(hi - med);
    const double dmax = (dlo > dhi) ? dlo : dhi;
    __syncthreads();
    const int rd[2] = {(n - 1) >> 1, n >> 1};
    double dsel[2];
    select_ranks<2, false>(st, s, n, 0.0, dmax, rd, dsel, bc, par);
    if (bc.tid == 0) {
        double mad = (n & 1) ? dsel[1] : (dsel[0] + dsel[1]) / 2.0;
        if (mad < kFeatEps) mad = kFeatEps;
        double competition = 0.0, difficulty = 0.0;
        if (n >= 2) {
            competition = gap / ((hi - lo) + kFeatEps);
            difficulty = 1.0 / ((hi - lo) / (double)(n - 1) + kFeatEps);
        }
        const double m = (n > 1) ? (double)n : 1.0;
        float *f = r.feat;
        f[0] = (float)lo;
        f[1] = (float)hi;
        f[2] = (float)mean;
        f[3] = (float)sqrt(sq / n);
        f[4] = (float)mad;
        f[5] = (float)ent;
        f[6] = (float)gap;
        f[7] = (float)competition;
        f[8] = (float)kmean;
        f[9] = (float)kstd;
        f[10] = (float)difficulty;
        f[11] = (float)((double)(cnts & 0xffff) / m);
        f[12] = (float)((double)(cnts >> 16) / m);
        for (int q = 0; q < 8; ++q) f[13 + q] = r.pos[q];
    }
}

__global__ void __launch_bounds__(kSweepThreads, 6) row_features_kernel(FeatureParams p, int npad)
{
    const int b = blockIdx.y, i = blockIdx.x, n = p.n;
    const size_t o = (size_t)b * n + i;
    FeatureRow r;
    r.row = p.C + o * n;
    r.cm = p.colmin + (size_t)b * n;
    r.pos = p.posenc + (size_t)i * 8;
    r.feat = p.feat + o * 21;
    r.topk = p.topk ? p.topk + o * 16 : nullptr;
    r.cost32 = nullptr;
    r.n = n;
    row_features_body<false>(r, npad);
}

// Ragged batch (ragged_batch.hpp): workgroup (i, b) owns row i of the padded [N] rows of instance b.
// A row of the prefix runs the body above at n = n_b; a padded row (i >= n_b, or every row of an
// instance whose size is outside 1..N) writes its zeros and +inf and leaves before the first barrier.
// The exit depends on blockIdx and sizes[b] only: workgroup-uniform.
__global__ void __launch_bounds__(kSweepThreads, 6) row_features_ragged_kernel(RaggedBatch g, RaggedFeatureOut o,
                                                                               int npad)
{
    const int b = blockIdx.y, i = blockIdx.x, N = g.N, tid = threadIdx.x;
    const int n = ragged_size(g, b);
    const size_t orow = (size_t)b * N + i;
    if (i == 0 && tid == 0) o.ret[b] = n ? 0 : 2;
    if (tid == 0 && o.mask) o.mask[orow] = i < n;
    if (o.cost32) {  // the zeros right of the prefix, or the whole padded row
        float *c = o.cost32 + orow * N;
        for (int j = (i < n ? n : 0) + tid; j < N; j += kSweepThreads) c[j] = 0.0f;
    }
    if (i >= n) {
        if (tid < 21) o.feat[orow * 21 + tid] = 0.0f;
        if (tid < 16 && o.topk) o.topk[orow * 16 + tid] = __builtin_inff();
        return;
    }
    FeatureRow r;
    r.row = g.C + g.offsets[b] + (size_t)i * (g.ld ? g.ld : n);
    r.cm = o.colmin + (size_t)b * N;
    r.pos = o.posenc + ((size_t)o.pos_off[b] + i) * 8;
    r.feat = o.feat + orow * 21;
    r.topk = o.topk ? o.topk + orow * 16 : nullptr;
    r.cost32 = o.cost32 ? o.cost32 + orow * N : nullptr;
    r.n = n;
    row_features_body<true>(r, npad);
}

}  // namespace

// One launch instead of two device-to-device copies and two memsets in front of the prelude: the
// working copies of the seeds, the per-instance flags and the helper ring.  (A kernel is also what
// a captured HIP graph replays most reliably: the runtime's memset nodes were seen to leave stale
// flags behind on replay, tools/diag_graph.py.)
__global__ void __launch_bounds__(kSweepThreads)
seed_prepare_kernel(const double *u_seed, const double *v_seed, double *u_work, double *v_work, size_t count,
                    int *flags, int n_flags, int *ring, int n_ring)
{
    const size_t gid = (size_t)blockIdx.x * kSweepThreads + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kSweepThreads;
    for (size_t k = gid; k < count; k += stride) {
        u_work[k] = u_seed[k];
        v_work[k] = v_seed[k];
    }
    for (size_t k = gid; k < (size_t)n_flags; k += stride) flags[k] = 0;
    for (size_t k = gid; k < (size_t)n_ring; k += stride) ring[k] = 0;
}

hipError_t launch_seed_prepare(const double *u_seed, const double *v_seed, double *u_work, double *v_work,
                               size_t count, int *flags, int n_flags, int *ring, int n_ring, hipStream_t stream)
{
    size_t blocks = (count + kSweepThreads - 1) / kSweepThreads;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(seed_prepare_kernel, dim3((unsigned)blocks), dim3(kSweepThreads), 0, stream, u_seed, v_seed,
                       u_work, v_work, count, flags, n_flags, ring, n_ring);
    return hipGetLastError();
}

// The same for a ragged batch, [batch][N] throughout: the seeds of the prefix of every instance (the padding
// is never read), the flags, and the results an instance keeps when no solver launch takes it -- x, y -1
// everywhere (the solver writes the prefix), ret 2 (a size outside 1..N), stats 0.
__global__ void __launch_bounds__(kSweepThreads)
seed_prepare_ragged_kernel(RaggedBatch g, const double *u_seed, const double *v_seed, double *u_work, double *v_work,
                           int *flags, long long *x, long long *y, int *ret, long long *stats)
{
    const int b = blockIdx.y, j = blockIdx.x * kSweepThreads + threadIdx.x, N = g.N;
    const int n = ragged_size(g, b);
    const size_t o = (size_t)b * N + j;
    if (j < n) {
        u_work[o] = u_seed[o];
        v_work[o] = v_seed[o];
    }
    if (j < N) {
        x[o] = -1;
        y[o] = -1;
    }
    if (j == 0) {
        flags[b] = 0;
        ret[b] = 2;
    }
    if (stats && j < kStatsPerInstance) stats[(size_t)b * kStatsPerInstance + j] = 0;
}

hipError_t launch_seed_prepare_ragged(const RaggedBatch &g, const double *u_seed, const double *v_seed, double *u_work,
                                      double *v_work, int *flags, long long *x, long long *y, int *ret,
                                      long long *stats, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seed_prepare_ragged_kernel, dim3((g.N + kSweepThreads - 1) / kSweepThreads, g.batch),
                       dim3(kSweepThreads), 0, stream, g, u_seed, v_seed, u_work, v_work, flags, x, y, ret, stats);
    return hipGetLastError();
}

hipError_t launch_prelude(const PreludeParams &p, hipStream_t stream)
{
    if (p.n > 16384) return hipErrorInvalidValue;
    const dim3 grid(p.n, p.batch), block(kSweepThreads);
    if (p.n <= 8 * kSweepThreads)
        hipLaunchKernelGGL(prelude_kernel<8>, grid, block, 0, stream, p);
    else if (p.n <= 16 * kSweepThreads)
        hipLaunchKernelGGL(prelude_kernel<16>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(prelude_kernel<0>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_projection(const double *C, int n, int batch, double *u, double *v,
                             const int *viol_cnt, int *inst_flags, double eps, hipStream_t stream)
{
    hipLaunchKernelGGL(projection_kernel, dim3(batch), dim3(kSweepThreads), 0, stream, C, n, u, v,
                       viol_cnt, inst_flags, eps);
    return hipGetLastError();
}

// p.n == g.N, p.batch == g.batch; p.C is not read.  The register-resident variant is chosen by N.
hipError_t launch_prelude_ragged(const PreludeParams &p, const RaggedBatch &g, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N) || p.n != g.N) return hipErrorInvalidValue;
    const dim3 grid(g.N, g.batch), block(kSweepThreads);
    if (g.N <= 8 * kSweepThreads)
        hipLaunchKernelGGL(prelude_ragged_kernel<8>, grid, block, 0, stream, p, g);
    else if (g.N <= 16 * kSweepThreads)
        hipLaunchKernelGGL(prelude_ragged_kernel<16>, grid, block, 0, stream, p, g);
    else
        hipLaunchKernelGGL(prelude_ragged_kernel<0>, grid, block, 0, stream, p, g);
    return hipGetLastError();
}

hipError_t launch_projection_ragged(const RaggedBatch &g, double *u, double *v, const int *viol_cnt, int *inst_flags,
                                    double eps, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(projection_ragged_kernel, dim3(g.batch), dim3(kSweepThreads), 0, stream, g, u, v, viol_cnt,
                       inst_flags, eps);
    return hipGetLastError();
}

int colmin_chunks(int n, int batch)
{
    const int coltiles = (n + 2 * kSweepThreads - 1) / (2 * kSweepThreads);
    int chunks = (2048 + batch * coltiles - 1) / (batch * coltiles);
    const int max_chunks = (n + 31) / 32;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < 1) chunks = 1;
    return chunks;
}

static hipError_t colmin_impl(const double *C, int n, int batch, const double *u, double *out,
                              double *partial, int final_mode, hipStream_t stream)
{
    const int chunks = colmin_chunks(n, batch);
    const int rows_per = (n + chunks - 1) / chunks;
    const bool pair = (n % 2) == 0 && (reinterpret_cast<uintptr_t>(C) % 16) == 0;
    const int cols_per_block = kSweepThreads * (pair ? 2 : 1);
    dim3 grid((n + cols_per_block - 1) / cols_per_block, chunks, batch);
    using Kernel = decltype(&colmin_partial_kernel<false, false>);
    static constexpr Kernel kPartial[2][2] = {{colmin_partial_kernel<false, false>, colmin_partial_kernel<false, true>},
                                              {colmin_partial_kernel<true, false>, colmin_partial_kernel<true, true>}};
    hipLaunchKernelGGL(kPartial[u != nullptr][pair], grid, dim3(kSweepThreads), 0, stream, C, n, u, partial, rows_per,
                       chunks);
    hipLaunchKernelGGL(colmin_final_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, stream,
                       partial, n, chunks, out, final_mode);
    return hipGetLastError();
}

hipError_t launch_colmin(const double *C, int n, int batch, const double *u, double *out,
                         double *partial, hipStream_t stream)
{
    return colmin_impl(C, n, batch, u, out, partial, 0, stream);
}

hipError_t launch_cap_cols(const double *C, int n, int batch, const double *u, double *v,
                           double *partial, hipStream_t stream)
{
    return colmin_impl(C, n, batch, u, v, partial, 1, stream);
}

hipError_t launch_rowmin(const double *C, int n, int batch, const double *v, double *out,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(rowmin_kernel, dim3(n, batch), dim3(kSweepThreads), 0, stream, C, n,
                       (const double *)nullptr, v, out, 0);
    return hipGetLastError();
}

hipError_t launch_cap_rows(const double *C, int n, int batch, double *u, const double *v,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(rowmin_kernel, dim3(n, batch), dim3(kSweepThreads), 0, stream, C, n,
                       (const double *)nullptr, v, u, 1);
    return hipGetLastError();
}

hipError_t launch_reduced_min(const double *C, int n, int batch, const double *u, const double *v,
                              double *gmin_partial, double *gmin, hipStream_t stream)
{
    hipLaunchKernelGGL(rowmin_kernel, dim3(n, batch), dim3(kSweepThreads), 0, stream, C, n, u, v,
                       gmin_partial, 2);
    hipLaunchKernelGGL(vecmin_kernel, dim3(batch), dim3(kSweepThreads), 0, stream, gmin_partial, n, gmin);
    return hipGetLastError();
}

hipError_t launch_reduce_costs(const double *C, int n, int batch, const double *u, const double *v,
                               const double *gmin, int shift_nonneg, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(reduce_costs_kernel, dim3(n, batch), dim3(kSweepThreads), 0, stream, C, n, u, v,
                       gmin, shift_nonneg, out);
    return hipGetLastError();
}

// exp(-(x - lo)) is not kept in LDS between the entropy passes: the closed form needs it once, the
// element-wise path recomputes it, and the 8 n bytes saved let 6-7 workgroups share a CU
// (measured: 1.29 -> 1.02 ms for 32 x 2048 rows together with the 6-waves-per-SIMD bound)
static size_t row_features_lds(int npad)
{
    return sizeof(BlockExchange) + sizeof(double) * (size_t)npad + sizeof(SelectState) +
           (size_t)npad;  // + one bucket byte per element
}

hipError_t launch_row_features(const FeatureParams &p, hipStream_t stream)
{
    if (p.n > 16384 || p.n < 1) return hipErrorInvalidValue;
    const int npad = (p.n + 1) & ~1;
    const size_t lds = row_features_lds(npad);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(row_features_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(row_features_kernel, dim3(p.n, p.batch), dim3(kSweepThreads), lds, stream, p, npad);
    return hipGetLastError();
}

// LDS is sized for N: the rows of one launch share one size, whatever their instance's n_b.
hipError_t launch_row_features_ragged(const RaggedBatch &g, const RaggedFeatureOut &o, hipStream_t stream)
{
    if (check_ragged_dims(g.batch, g.N)) return hipErrorInvalidValue;
    const int npad = (g.N + 1) & ~1;
    const size_t lds = row_features_lds(npad);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(row_features_ragged_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(row_features_ragged_kernel, dim3(g.N, g.batch), dim3(kSweepThreads), lds, stream, g, o, npad);
    return hipGetLastError();
}

}  // namespace lapwarm
