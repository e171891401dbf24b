// oracle_duals.hpp -- launchers and workspace slots of the oracle-duals kernels (oracle_duals.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace lapwarm {

constexpr int kOracleMaxN = 16384;
constexpr int kOracleReplayMaxN = 2048;  // largest n whose unsettled instances are replayed exactly
// per-instance results (the ret codes of lapwarm_oracle_duals_batched) and internal states
constexpr int kOracleOk = 0, kOracleNegativeCycle = 1, kOracleInfeasible = 2, kOracleSlackness = 3,
              kOracleNotPermutation = 4, kOracleNonFinite = 5;
// ragged call only: the size is outside 1..N or wider than the row stride (ragged_size gives 0); no work is done
constexpr int kOracleEmpty = 6;
constexpr int kOracleDone = 100, kOracleReplay = 101;  // status 0: still sweeping
// per-instance int slots of the workspace
constexpr int kOdStatus = 0, kOdCount0 = 1, kOdCount1 = 2, kOdSweeps = 3, kOdDepth = 4, kOdRowsRead = 5,
              kOdReplayed = 6, kOdSlackBad = 7, kOdInstInts = 16;
// A ragged batch sets offsets, sizes and ld (ragged_batch.hpp) and n = N, the padded width: every [batch][n]
// array below then has the row stride N and instance b uses its prefix n_b.  sizes == nullptr: uniform.
struct OracleParams {
    const double *C;
    int n, batch, chunks, pair;
    const long long *offsets = nullptr;
    const int *sizes = nullptr;
    int ld = 0;
    const int *rows, *cols;  // [batch][n] pairs in the caller's order
    int *x, *y;              // [batch][n] row -> col, col -> row
    double *cxx;             // [batch][n] C[i][x_i]
    double *v0, *v1;         // [batch][n] the two Jacobi buffers
    int *pred;               // [batch][n] row that last lowered v_j, or -1
    int *lrow;               // [2][batch][n] active rows of the current / next sweep
    double *lsrc;            // [2][batch][n] their source values v[x_i]
    double *pval;            // [batch][chunks][n] partial column minima
    int *parg;               // [batch][chunks][n] their rows
    int *inst;               // [batch][kOdInstInts]
};
int oracle_chunks(int n, int batch);
hipError_t launch_oracle_init(const OracleParams &p, hipStream_t stream);
// sweep s (0-based, the same for every instance of the batch; a ragged instance skips s >= n_b - 1)
hipError_t launch_oracle_sweep(const OracleParams &p, int s, hipStream_t stream);
// after s sweeps: stop the converged, find predecessor cycles; `last` hands the unsettled to the
// replay; `running` (zeroed by the caller) receives the number of instances that go on sweeping
// (ragged: s is the batch's sweep number and `last` is decided per instance on the device, s >= n_b - 1)
hipError_t launch_oracle_check(const OracleParams &p, int s, int last, int *running, hipStream_t stream);
// replay (n <= kOracleReplayMaxN), u/v with the gauge, reduced-cost minimum, ret and counters
hipError_t launch_oracle_finish(const OracleParams &p, double tol, double *u, double *v, double *rowpart,
                                double *gmin, int *ret, int *sweeps, hipStream_t stream);

}  // namespace lapwarm
