// prune_price.hpp -- pruning and pricing of dense cost rows into CSR (prune_price.hip): the device half of the
// exact dense solve through sparse LAPMOD.  One grow step keeps, per row of a ragged batch, the current columns of
// the row plus the at most m absent columns with the smallest key below the row's bound, and writes the next CSR.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ragged_batch.hpp"

namespace lapwarm {

constexpr int kPruneItems = 16;     // columns a thread holds at most: 1024 threads cover a row of kMaxN
constexpr int kPruneMaxThreads = 1024;
constexpr int kPruneMaxM = 256;
static_assert(kPruneItems * kPruneMaxThreads >= kMaxN, "a workgroup holds a whole row in registers");

// ret [batch] of a grow step
enum PruneRet {
    kPruneOk = 0,
    kPruneInadmissible = 3,  // a cost outside [0, LARGE) or NaN, a key vector entry that is not finite, an x_i or an
                             // input column outside 0..n-1, input row starts that do not ascend: nothing is written
    kPruneEmpty = 4,         // the ragged layer treats the instance as empty (ragged_size): no work
    kPruneNoRoom = 5,        // the next CSR does not fit cap_out[b]: nothing of it is written
};

// Per row, [batch][N] each: what the count pass leaves for the scan and the fill pass.
struct PruneWs {
    unsigned long long *thr;  // image of the largest key taken (all ones: every eligible entry is taken)
    int *ties;                // how many of the eligible entries with that image are taken, lowest column first
    int *len;                 // length of the row in the next CSR
    int *nelig;               // |E_i|
    int *bad;                 // the row saw something inadmissible
    size_t bytes;
};

struct PruneGrow {
    const double *key;           // [batch][N] seed or v, or null: key_ij = C_ij - key_j (C_ij without)
    const int *x;                // [batch][N] or null: bound_i = C[i][x_i] - key[x_i] (+inf without)
    const int *kk_in, *ii_in;    // the current CSR, or null: every row holds its diagonal only
    const long long *nnz_off_in, *row_off_in;
    int m;
    double *cc_out;              // null: price only (added, viol and ret; no CSR is written)
    int *kk_out, *ii_out;
    const long long *nnz_off_out, *row_off_out, *cap_out;
    long long *added, *viol;     // [batch]
    int *ret;                    // [batch] PruneRet
};

// count pass, one scan per instance, fill pass: dims checked by the caller
hipError_t launch_prune_grow(const RaggedBatch &g, const PruneGrow &p, const PruneWs &w, hipStream_t stream);

// u_i = C[i][x_i] - v[x_i] and cost = sum_i C[i][x_i] (serially, ascending i) of the instances with ret 0 or 2; the
// tails of u and v are zeroed; any other ret (or an x_i outside 0..n-1) gives u, v all 0 and cost inf.
hipError_t launch_prune_finish(const RaggedBatch &g, const int *x, double *v, const int *ret, double *u, double *cost,
                               hipStream_t stream);

}  // namespace lapwarm
