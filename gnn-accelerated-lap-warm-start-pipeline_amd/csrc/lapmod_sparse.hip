// lapmod_sparse.hip -- sparse LAPMOD on the device: LAP/_lapjv_cpp/lapmod.cpp restated for one wave per instance.
//
// One workgroup of 64 lanes solves one CSR instance; a launch takes a batch of instances of different n and nnz.
// The solver state (lapmod_sparse.hpp) lives in LDS up to lapmod_lds_max_n() and in the caller's workspace above
// it; cc and kk are read from HBM where they lie.  x, y and the final v are those of the reference bit for bit:
// only fp64 adds, subtracts and compares, in the reference's association order ((cc - v[j]) - h).
//
// What runs across the lanes of the wave, and what stays serial ("Sparse LAPMOD"):
//   column minima      atomic minimum of the bit patterns (costs are >= 0), then the smallest row among the
//                      entries equal to it: the reference's strict `<` over ascending rows
//   backward pass      per-row maximum of the claiming columns; the others lose their row
//   reduction transfer rows in serial order (row i reads v[j2] that earlier rows lowered), wave minimum per row
//   ARR                free rows in serial order, lexicographic (value, position) top-2 per row
//   find_path_sparse_2 minima, list appends (ballot + prefix: order kept), price updates across lanes; the
//                      SCAN list one column at a time
//   find_path_sparse_1 the find step and the swaps of cols[] on one lane (each swap reads what the previous one
//                      wrote); the relaxation of the TODO columns across lanes
// Every loop is bounded by n and nnz; an instance that exceeds a bound ends with a negative ret.
#include "lapmod_sparse.hpp"

#include <atomic>

#include "device_utils.hpp"

namespace lapwarm {

namespace {

constexpr int kIntMax = 0x7fffffff;

struct Lm {
    int n, lane;
    const double *cc;
    const int *kk, *ii;
    double *v, *d;
    int *x, *y, *pred, *fr, *la, *lb, *lc, *rev;
    unsigned *done, *added;
    long long finds, scans;
};

__device__ __forceinline__ bool bit_get(const unsigned *b, int j) { return (b[j >> 5] >> (j & 31)) & 1u; }
__device__ __forceinline__ void bit_set(unsigned *b, int j) { atomicOr(&b[j >> 5], 1u << (j & 31)); }
__device__ __forceinline__ int rank_below(unsigned long long m, int lane)
{
    return __popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ int first_lane(unsigned long long m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int last_lane(unsigned long long m) { return 63 - __builtin_clzll(m); }

// _ccrrt_sparse: returns the number of free rows, listed ascending in fr
__device__ int lm_ccrrt(Lm &s)
{
    const int n = s.n, lane = s.lane;
    unsigned long long *vbits = reinterpret_cast<unsigned long long *>(s.v);
    for (int i = lane; i < n; i += kWave) {
        s.x[i] = -1;
        s.v[i] = kLarge;
        s.y[i] = kIntMax;
    }
    for (int w = lane; w < (n + 31) / 32; w += kWave) s.done[w] = 0;  // here: rows that are not `unique`
    __syncthreads();
    // v[j] = the smallest entry of column j (costs are >= 0: their bit patterns order as integers)
    for (int i = lane; i < n; i += kWave) {
        const int re = s.ii[i + 1];
        for (int k = s.ii[i]; k < re; ++k)
            atomicMin(&vbits[s.kk[k]], (unsigned long long)__double_as_longlong(s.cc[k] + 0.0));
    }
    __syncthreads();
    // y[j] = the smallest row that holds it (strict `<`, rows ascending)
    for (int i = lane; i < n; i += kWave) {
        const int re = s.ii[i + 1];
        for (int k = s.ii[i]; k < re; ++k) {
            const int j = s.kk[k];
            if ((unsigned long long)__double_as_longlong(s.cc[k] + 0.0) == vbits[j]) atomicMin(&s.y[j], i);
        }
    }
    __syncthreads();
    for (int j = lane; j < n; j += kWave)
        if (s.y[j] == kIntMax) s.y[j] = 0;  // an empty column keeps the initial y = 0
    __syncthreads();
    // backward pass j = n-1..0: the largest claiming column takes the row
    for (int j = lane; j < n; j += kWave) atomicMax(&s.x[s.y[j]], j);
    __syncthreads();
    for (int j = lane; j < n; j += kWave) {
        const int i = s.y[j];
        if (s.x[i] != j) {
            bit_set(s.done, i);
            s.y[j] = -1;
        }
    }
    __syncthreads();
    int nfree = 0;
    for (int base = 0; base < n; base += kWave) {
        const int i = base + lane;
        const bool act = i < n;
        const int xi = act ? s.x[i] : 0;
        const int rs0 = act ? s.ii[i] : 0, re0 = act ? s.ii[i + 1] : 0;
        const bool is_free = act && xi < 0;
        const unsigned long long fm = __ballot(is_free);
        if (is_free) s.fr[nfree + rank_below(fm, lane)] = i;
        nfree += __popcll(fm);
        unsigned long long tm = __ballot(act && xi >= 0 && !bit_get(s.done, i) && re0 - rs0 > 1);
        while (tm) {  // reduction transfer, rows in order
            const int l = first_lane(tm);
            tm &= tm - 1;
            const int j = __shfl(xi, l, kWave), rs = __shfl(rs0, l, kWave), re = __shfl(re0, l, kWave);
            double m = kLarge;
            for (int k = rs + lane; k < re; k += kWave) {
                const int j2 = s.kk[k];
                if (j2 != j) m = dmin(m, s.cc[k] - s.v[j2]);
            }
            m = wave_min(m);
            if (lane == 0) s.v[j] = s.v[j] - m;
            __syncthreads();
        }
    }
    __syncthreads();
    return nfree;
}

// _carr_sparse: one pass over the free rows; returns the new number of free rows
__device__ int lm_arr(Lm &s, int nfree, long long *iters, int *err)
{
    const int n = s.n, lane = s.lane;
    unsigned current = 0, rr_cnt = 0;
    int new_free = 0;
    // --current needs rr_cnt < current * n <= n * n, every other iteration advances current
    const unsigned long long bound = (unsigned long long)n * (unsigned)n + 2ull * (unsigned)n + 2ull;
    unsigned long long it = 0;
    while (current < (unsigned)nfree) {
        if (++it > bound) {
            *err = -3;
            break;
        }
        rr_cnt++;
        const int free_i = s.fr[current++];
        const int rs = s.ii[free_i], re = s.ii[free_i + 1];
        int j1 = 0, j2 = -1;
        double v1 = kLarge, v2 = kLarge;
        if (re - rs > 0) {
            // The serial loop seeds (j1, v1) with the first entry whatever its value, and (j2, v2) with (-1, LARGE):
            // a sentinel that sits between position 0 and position 1.  With a first value <= LARGE the result is
            // the lexicographic (value, position) top-2 of the entries and the sentinel.  With a first value above
            // LARGE the serial loop ignores every entry until the first one below LARGE (position p), after which
            // the sentinel is gone: top-2 of entry 0 and the entries from p on.
            const int ja = s.kk[rs];
            const double a0 = s.cc[rs] - s.v[ja];
            int p = 1;
            bool sentinel = true;
            if (a0 > kLarge) {
                p = kIntMax;
                for (int base = rs + 1; base < re && p == kIntMax; base += kWave) {
                    const int k = base + lane;
                    const bool below = k < re && (s.cc[k] - s.v[s.kk[k]]) < kLarge;
                    const unsigned long long m = __ballot(below);
                    if (m) p = base - rs + first_lane(m);
                }
                sentinel = false;
            }
            if (p == kIntMax) {
                j1 = ja;
                v1 = a0;
            } else {
                Top2 t = top2_empty();
                for (int k = rs + lane; k < re; k += kWave) {
                    const int pos = k - rs;
                    if (pos == 0 || pos >= p) top2_push(t, s.cc[k] - s.v[s.kk[k]], 2 * pos);
                }
                t = wave_top2(t);
                if (sentinel) top2_push(t, kLarge, 1);
                v1 = t.a1;
                j1 = s.kk[rs + (t.i1 >> 1)];
                if (t.i2 != 1 && t.i2 != kIntMax) {
                    v2 = t.a2;
                    j2 = s.kk[rs + (t.i2 >> 1)];
                }
            }
        }
        int i0 = s.y[j1];
        const double vj1 = s.v[j1];
        const double v1_new = vj1 - (v2 - v1);
        const bool v1_lowers = v1_new < vj1;
        __syncthreads();  // every lane has read fr, v and y before lane 0 writes them
        if (rr_cnt < current * (unsigned)n) {
            if (v1_lowers) {
                if (lane == 0) s.v[j1] = v1_new;
            } else if (i0 >= 0 && j2 >= 0) {
                j1 = j2;
                i0 = s.y[j2];
            }
            if (i0 >= 0) {
                if (v1_lowers) {
                    --current;
                    if (lane == 0) s.fr[current] = i0;
                } else {
                    if (lane == 0) s.fr[new_free] = i0;
                    new_free++;
                }
            }
        } else if (i0 >= 0) {
            if (lane == 0) s.fr[new_free] = i0;
            new_free++;
        }
        if (lane == 0) {
            s.x[free_i] = j1;
            s.y[j1] = free_i;
        }
        __syncthreads();
    }
    *iters += (long long)it;
    return new_free;
}

// d = LARGE, pred = start_i, then d[j] = cc - v[j] over the row of start_i
__device__ void lm_path_init(Lm &s, int start_i, bool lists)
{
    const int n = s.n, lane = s.lane;
    for (int i = lane; i < n; i += kWave) {
        s.d[i] = kLarge;
        s.pred[i] = start_i;
        if (!lists) s.la[i] = i;
    }
    if (lists)
        for (int w = lane; w < (n + 31) / 32; w += kWave) {
            s.done[w] = 0;
            s.added[w] = 0;
        }
    __syncthreads();
    const int rs = s.ii[start_i], re = s.ii[start_i + 1];
    for (int k = rs + lane; k < re; k += kWave) {
        const int j = s.kk[k];
        s.d[j] = s.cc[k] - s.v[j];
        if (lists) {
            s.lb[k - rs] = j;
            bit_set(s.added, j);
        }
    }
    __syncthreads();
}

// find_path_sparse_2.  rev_kk is all -1 on entry and on exit.  Returns final_j, or -1 with *err set: 1 when the
// problem has no perfect matching (no candidate left, or the scanned column is absent from its row: the
// reference reads outside its arrays in both cases), negative when a bound is exceeded.
__device__ int lm_find_path_2(Lm &s, int start_i, int *err)
{
    const int n = s.n, lane = s.lane;
    int *scan = s.la, *todo = s.lb, *ready = s.lc;
    lm_path_init(s, start_i, true);
    int n_todo = s.ii[start_i + 1] - s.ii[start_i];
    int lo = 0, hi = 0, n_ready = 0, final_j = -1;
    int rounds = 0;
    while (final_j == -1) {
        if (++rounds > n + 2) {  // every round without a result takes at least one column off SCAN for good
            *err = -4;
            return -1;
        }
        if (lo == hi) {
            s.finds++;
            double m = pos_inf();
            for (int k = lane; k < n_todo; k += kWave) {
                const int j = todo[k];
                if (!bit_get(s.done, j)) m = dmin(m, s.d[j]);
            }
            m = wave_min(m);
            if (!(m <= kLarge)) {  // _find_sparse_2 returns 0
                *err = 1;
                return -1;
            }
            lo = 0;
            hi = 0;
            for (int base = 0; base < n_todo; base += kWave) {
                const int k = base + lane;
                const int j = k < n_todo ? todo[k] : 0;
                const bool sel = k < n_todo && !bit_get(s.done, j) && s.d[j] == m;
                const unsigned long long bm = __ballot(sel);
                if (sel) scan[hi + rank_below(bm, lane)] = j;
                hi += __popcll(bm);
            }
            __syncthreads();
            for (int base = 0; base < hi; base += kWave) {  // the last unassigned one wins, the others are done
                const int k = base + lane;
                const int j = k < hi ? scan[k] : 0;
                const bool unassigned = k < hi && s.y[j] < 0;
                const unsigned long long bm = __ballot(unassigned);
                if (bm) final_j = __shfl(j, last_lane(bm), kWave);
                if (k < hi && !unassigned) bit_set(s.done, j);
            }
            __syncthreads();
        }
        if (final_j == -1) {
            const int lo_in = lo, n_ready_in = n_ready;  // a hit inside the scan returns without storing these
            while (lo != hi) {
                const int j = scan[lo++];
                const int i = s.y[j];
                if (n_ready >= n || i < 0) {
                    *err = -4;
                    return -1;
                }
                if (lane == 0) ready[n_ready] = j;
                n_ready++;
                s.scans++;
                const double mind = s.d[j];
                const int rs = s.ii[i], re = s.ii[i + 1];
                for (int k = rs + lane; k < re; k += kWave) s.rev[s.kk[k]] = k;
                __syncthreads();
                const int kj = s.rev[j];
                int found = -1, over = 0;
                if (kj != -1) {
                    const double h = (s.cc[kj] - s.v[j]) - mind;
                    for (int base = rs; base < re; base += kWave) {
                        const int k = base + lane;
                        const int jj = k < re ? s.kk[k] : 0;
                        const bool live = k < re && !bit_get(s.done, jj);
                        const double cred = live ? (s.cc[k] - s.v[jj]) - h : 0.0;
                        const bool upd = live && cred < s.d[jj];
                        const bool hit = upd && cred <= mind;
                        const unsigned long long fb = __ballot(hit && s.y[jj] < 0);
                        const int L = fb ? first_lane(fb) : kWave;  // the serial loop returns at this entry
                        if (upd && lane <= L) {
                            s.d[jj] = cred;
                            s.pred[jj] = i;
                        }
                        const bool to_scan = hit && lane < L;
                        const bool to_todo = upd && !hit && lane < L && !bit_get(s.added, jj);
                        const unsigned long long sm = __ballot(to_scan), tm = __ballot(to_todo);
                        if (hi + __popcll(sm) > n || n_todo + __popcll(tm) > n) {
                            over = 1;
                            break;
                        }
                        if (to_scan) {
                            scan[hi + rank_below(sm, lane)] = jj;
                            bit_set(s.done, jj);
                        }
                        if (to_todo) {
                            todo[n_todo + rank_below(tm, lane)] = jj;
                            bit_set(s.added, jj);
                        }
                        hi += __popcll(sm);
                        n_todo += __popcll(tm);
                        if (fb) {
                            found = __shfl(jj, L, kWave);
                            break;
                        }
                    }
                }
                __syncthreads();
                for (int k = rs + lane; k < re; k += kWave) s.rev[s.kk[k]] = -1;
                __syncthreads();
                if (kj == -1 || over) {
                    *err = over ? -4 : 1;
                    return -1;
                }
                if (found >= 0) {
                    final_j = found;
                    lo = lo_in;
                    n_ready = n_ready_in;
                    break;
                }
            }
        }
    }
    const double mind = s.d[scan[lo]];
    for (int k = lane; k < n_ready; k += kWave) {
        const int j = ready[k];
        s.v[j] = s.v[j] + (s.d[j] - mind);
    }
    __syncthreads();
    return final_j;
}

// find_path_sparse_1.  Returns final_j, or -1 with *err set: 1 when the smallest d of a find step is >= LARGE
// (no perfect matching), negative when a bound is exceeded.
__device__ int lm_find_path_1(Lm &s, int start_i, int *err)
{
    const int n = s.n, lane = s.lane;
    int *cols = s.la;
    lm_path_init(s, start_i, false);
    int lo = 0, hi = 0, n_ready = 0, final_j = -1;
    int rounds = 0;
    while (final_j == -1) {
        if (++rounds > n + 2 || lo >= n) {
            *err = -5;
            return -1;
        }
        if (lo == hi) {
            s.finds++;
            n_ready = lo;
            int nh = 0;
            if (lane == 0) {  // _find_sparse_1: every swap reads what the previous one wrote
                nh = lo + 1;
                double mind = s.d[cols[lo]];
                for (int k = nh; k < n; ++k) {
                    const int j = cols[k];
                    const double dj = s.d[j];
                    if (dj <= mind) {
                        if (dj < mind) {
                            nh = lo;
                            mind = dj;
                        }
                        cols[k] = cols[nh];
                        cols[nh++] = j;
                    }
                }
            }
            hi = __shfl(nh, 0, kWave);
            __syncthreads();
            if (!(s.d[cols[lo]] < kLarge)) {
                *err = 1;
                return -1;
            }
            for (int base = lo; base < hi; base += kWave) {
                const int k = base + lane;
                const int j = k < hi ? cols[k] : 0;
                const unsigned long long bm = __ballot(k < hi && s.y[j] < 0);
                if (bm) final_j = __shfl(j, last_lane(bm), kWave);
            }
        }
        if (final_j == -1) {
            const int lo_in = lo;  // a hit inside the scan returns without storing lo
            while (lo != hi) {
                const int j = cols[lo++];
                const int i = s.y[j];
                if (i < 0) {
                    *err = -5;
                    return -1;
                }
                s.scans++;
                const double mind = s.d[j];
                for (int k = lane; k < n; k += kWave) s.rev[k] = -1;
                __syncthreads();
                const int rs = s.ii[i], re = s.ii[i + 1];
                for (int k = rs + lane; k < re; k += kWave) s.rev[s.kk[k]] = k;
                __syncthreads();
                const int kj = s.rev[j];
                if (kj == -1) continue;
                const double h = (s.cc[kj] - s.v[j]) - mind;
                int found = -1;
                for (int base = hi; base < n; base += kWave) {  // the TODO columns, in the order of cols[]
                    const int k = base + lane;
                    const int jj = k < n ? cols[k] : 0;
                    const int kq = k < n ? s.rev[jj] : -1;
                    const double cred = kq != -1 ? (s.cc[kq] - s.v[jj]) - h : 0.0;
                    const bool upd = kq != -1 && cred < s.d[jj];
                    const bool hit = upd && cred == mind;
                    const unsigned long long fb = __ballot(hit && s.y[jj] < 0);
                    const int L = fb ? first_lane(fb) : kWave;
                    if (upd && lane <= L) {
                        s.d[jj] = cred;
                        s.pred[jj] = i;
                    }
                    unsigned long long hm = __ballot(hit && lane < L);
                    __syncthreads();
                    int nh = hi;
                    if (lane == 0) {  // the swaps of the hits, in order; positions beyond k are never written
                        while (hm) {
                            const int kp = base + first_lane(hm);
                            hm &= hm - 1;
                            const int t = cols[kp];
                            cols[kp] = cols[nh];
                            cols[nh++] = t;
                        }
                    }
                    nh = __shfl(nh, 0, kWave);
                    __syncthreads();
                    // (base stays ahead of hi: hi grows by at most the hits below base + 64)
                    hi = nh;
                    if (fb) {
                        found = __shfl(jj, L, kWave);
                        break;
                    }
                }
                if (found >= 0) {
                    final_j = found;
                    lo = lo_in;
                    break;
                }
            }
        }
    }
    const double mind = s.d[cols[lo]];
    for (int k = lane; k < n_ready; k += kWave) {
        const int j = cols[k];
        s.v[j] = s.v[j] + (s.d[j] - mind);
    }
    __syncthreads();
    return final_j;
}

__global__ void __launch_bounds__(kLapmodThreads) lapmod_plan_kernel(LapmodParams p)
{
    const int lane = threadIdx.x;
    long long run = 0;
    for (int base = 0; base < p.batch; base += kWave) {
        const int b = base + lane;
        const int n = b < p.batch ? p.sizes[b] : 0;
        const long long bytes = (n > p.lds_n && n <= p.N) ? (long long)lapmod_state_bytes(n) : 0;
        long long incl = bytes;
        for (int sft = 1; sft < kWave; sft <<= 1) {
            const long long o = __shfl_up(incl, sft, kWave);
            if (lane >= sft) incl += o;
        }
        if (b < p.batch) p.ws_off[b] = run + incl - bytes;
        run += __shfl(incl, kWave - 1, kWave);
    }
}

__global__ void __launch_bounds__(kLapmodThreads) lapmod_kernel(LapmodParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    int *xo = p.x + (size_t)b * p.N, *yo = p.y + (size_t)b * p.N;
    double *vo = p.v ? p.v + (size_t)b * p.N : nullptr;
    long long *st = p.stats ? p.stats + (size_t)b * 32 : nullptr;
    for (int j = lane; j < p.N; j += kWave) {
        xo[j] = -1;
        yo[j] = -1;
        if (vo) vo[j] = __longlong_as_double(0x7ff8000000000000LL);
    }
    if (st && lane < 32) st[lane] = 0;
    const int n = p.sizes[b];
    if (n < 1 || n > p.N) {
        if (lane == 0) p.ret[b] = 2;
        return;
    }
    unsigned char *base = lm_lds;
    const bool in_lds = n <= p.lds_n;
    if (!in_lds) {
        const long long off = p.ws_off ? p.ws_off[b] : -1;
        if (off < 0 || (unsigned long long)off + lapmod_state_bytes(n) > p.ws_state_bytes) {
            if (lane == 0) p.ret[b] = 2;
            return;
        }
        base = p.ws_state + off;
    }
    Lm s;
    s.n = n;
    s.lane = lane;
    s.cc = p.cc + p.nnz_off[b];
    s.kk = p.kk + p.nnz_off[b];
    s.ii = p.ii + p.row_off[b];
    s.v = reinterpret_cast<double *>(base);
    s.d = s.v + n;
    s.x = reinterpret_cast<int *>(s.d + n);
    s.y = s.x + n;
    s.pred = s.y + n;
    s.fr = s.pred + n;
    s.la = s.fr + n;
    s.lb = s.la + n;
    s.lc = s.lb + n;
    s.rev = s.lc + n;
    s.done = reinterpret_cast<unsigned *>(s.rev + n);
    s.added = s.done + (n + 31) / 32;
    s.finds = s.scans = 0;

    // the input is checked before it indexes anything: row starts ascending from 0 with at most n entries a row,
    // columns inside 0..n-1, costs inside [0, LARGE)
    bool bad = false;
    for (int i = lane; i < n; i += kWave) {
        const int a = s.ii[i], e = s.ii[i + 1];
        bad |= e < a || e - a > n || (i == 0 && a != 0);
    }
    if (__ballot(bad)) {
        if (lane == 0) p.ret[b] = 2;
        return;
    }
    const int nnz = s.ii[n];
    for (int k = lane; k < nnz; k += kWave) {
        const int j = s.kk[k];
        const double c = s.cc[k];
        bad |= j < 0 || j >= n || !(c >= 0.0) || !(c < kLarge);
    }
    if (__ballot(bad)) {
        if (lane == 0) p.ret[b] = 2;
        return;
    }

    int err = 0;
    long long arr_iters = 0, paths = 0;
    int free_arr[2] = {-1, -1};
    int nfree = lm_ccrrt(s);
    const int free_ccrrt = nfree;
    for (int pass = 0; pass < 2 && nfree > 0 && err == 0; ++pass) {
        nfree = lm_arr(s, nfree, &arr_iters, &err);
        free_arr[pass] = nfree;
    }
    // get_better_find_path: one search for the whole matrix, in the reference's 32-bit arithmetic
    int search = p.fp_version;
    if (search == 3) search = ((unsigned)nnz / (double)((unsigned)n * (unsigned)n) > 0.25) ? 1 : 2;
    int ran = 0;
    if (nfree > 0 && err == 0) {
        ran = search;
        if (search == 2) {
            for (int k = lane; k < n; k += kWave) s.rev[k] = -1;
            __syncthreads();
        }
        for (int f = 0; f < nfree && err == 0; ++f) {
            const int free_i = s.fr[f];
            const int fj = search == 1 ? lm_find_path_1(s, free_i, &err) : lm_find_path_2(s, free_i, &err);
            if (err) break;
            paths++;
            int e = 0;
            if (lane == 0) {
                int i = -1, j = fj, k = 0;
                while (i != free_i) {
                    if (j < 0 || j >= n || ++k > n) {
                        e = -6;
                        break;
                    }
                    i = s.pred[j];
                    s.y[j] = i;
                    const int t = s.x[i];
                    s.x[i] = j;
                    j = t;
                }
            }
            err = __shfl(e, 0, kWave);
            __syncthreads();
        }
    }
    if (err == 0) {
        for (int j = lane; j < n; j += kWave) {
            xo[j] = s.x[j];
            yo[j] = s.y[j];
            if (vo) vo[j] = s.v[j];
        }
    }
    if (lane == 0) {
        p.ret[b] = err;
        if (st) {
            st[kLmFreeCcrrt] = free_ccrrt;
            st[kLmFreeArr1] = free_arr[0];
            st[kLmFreeArr2] = free_arr[1];
            st[kLmArrIters] = arr_iters;
            st[kLmPaths] = paths;
            st[kLmFinds] = s.finds;
            st[kLmScanSteps] = s.scans;
            st[kLmSearchRan] = ran;
            st[kLmN] = n;
            st[kLmNnz] = nnz;
            st[kLmStateInLds] = in_lds ? 1 : 0;
            st[kLmSearchPicked] = search;
        }
    }
}

}  // namespace

hipError_t launch_lapmod_plan(const LapmodParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(lapmod_plan_kernel, dim3(1), dim3(kLapmodThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_lapmod(const LapmodParams &p, hipStream_t stream)
{
    const size_t lds = lapmod_state_bytes(p.lds_n > 0 ? p.lds_n : 1);
    // more dynamic LDS than the 64 KB default has to be allowed once per process (and not inside a capture: the
    // first launch that needs it is the uncaptured warm-up every captured call has)
    static std::atomic<bool> raised{false};
    if (lds > 64 * 1024 && !raised.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lapmod_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLapmodLdsBytes);
        if (e != hipSuccess) return e;
        raised.store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(lapmod_kernel, dim3(p.batch), dim3(kLapmodThreads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace lapwarm
