// lapmod_sparse.hpp -- sparse LAPMOD (LAP/_lapjv_cpp/lapmod.cpp) for a batch of CSR problems of different n and
// nnz: one instance per workgroup of one wave (lapmod_sparse.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace lapwarm {

constexpr int kLapmodThreads = 64;           // one wave: every exchange is a lane exchange, no cross-wave step
// The reference evaluates `current * n` (up to n * n) and the n * n of the FP_DYNAMIC density in 32-bit unsigned
// arithmetic, which wraps from n = 65536 on; the ARR bound below assumes it does not.  Larger n are refused.
constexpr int kLapmodMaxN = 65535;
constexpr size_t kLapmodLdsBytes = 160 * 1024;

// slots of stats [batch][32]
enum LapmodStat {
    kLmFreeCcrrt = 0,   // free rows after column reduction and reduction transfer
    kLmFreeArr1 = 1,    // after the first ARR pass (-1: not run)
    kLmFreeArr2 = 2,    // after the second (-1: not run)
    kLmArrIters = 3,    // ARR iterations of both passes
    kLmPaths = 4,       // augmenting paths
    kLmFinds = 5,       // calls of the find step
    kLmScanSteps = 6,   // columns taken off the SCAN list
    kLmSearchRan = 7,   // 0: augmentation not reached, 1: find_path_sparse_1, 2: find_path_sparse_2
    kLmN = 8,
    kLmNnz = 9,
    kLmStateInLds = 10,
    kLmSearchPicked = 11,  // what fp_version selects for this matrix, run or not
};

// Per-instance solver state, in this order: v, d [n] fp64; x, y, pred, free_rows, list_a, list_b, list_c, rev_kk
// [n] int32 (list_a is cols of find_path_sparse_1 or scan of find_path_sparse_2, list_b todo, list_c ready); done,
// added [ceil(n / 32)] bitmaps.  Rounded up to 16 bytes.
__host__ __device__ inline size_t lapmod_state_bytes(int n)
{
    const size_t b = 16 * (size_t)n + 32 * (size_t)n + 8 * (size_t)((n + 31) / 32);
    return (b + 15) & ~(size_t)15;
}

// the largest n whose state fits the 160 KB of LDS
inline int lapmod_lds_max_n()
{
    int n = (int)(kLapmodLdsBytes / 48);
    while (n > 0 && lapmod_state_bytes(n) > kLapmodLdsBytes) --n;
    return n;
}

struct LapmodParams {
    const double *cc;          // concatenated values
    const int *kk;             // concatenated column indices
    const int *ii;             // concatenated row starts, n_b + 1 per instance, local
    const long long *nnz_off;  // [batch] start of instance b in cc and kk
    const long long *row_off;  // [batch] start of instance b in ii
    const int *sizes;          // [batch] device
    int batch, N, fp_version;
    int lds_n;                 // instances up to this size keep their state in LDS (the launch's dynamic LDS fits it)
    int *x, *y;                // [batch][N]
    double *v;                 // [batch][N] or null
    int *ret;                  // [batch]
    long long *stats;          // [batch][32] or null
    long long *ws_off;         // [batch] workspace: state offset of the instances above lds_n (null: there are none)
    unsigned char *ws_state;   // 16-byte aligned
    size_t ws_state_bytes;
};

// ws_off from the device sizes: one workgroup
hipError_t launch_lapmod_plan(const LapmodParams &p, hipStream_t stream);
hipError_t launch_lapmod(const LapmodParams &p, hipStream_t stream);

}  // namespace lapwarm
