"""Oracle duals on the GPU (reference: solvers/dual_computation.py:13-114).

`dual_from_matching_diff_constraints` rebuilds (u, v) from a full matching through
lapwarm_oracle_duals (csrc/oracle_duals.hip): frontier Jacobi sweeps of the difference
constraints, bit-identical to the reference's Gauss-Seidel Bellman-Ford whenever that loop
settles, and an exact replay of the loop where it might not.  Same exceptions and messages.

Deviations, documented:
  * the matching of `compute_oracle_duals` comes from `lap.lapjv` (bit-identical to the
    reference's lapjv), not SciPy's linear_sum_assignment.  Where the optimum is unique both give
    the same matching and the same bits; with ties another optimal matching may be chosen, and the
    duals are still optimal.
  * non-square C, partial matchings, matchings that are not permutations and non-finite C raise
    ValueError.
"""
from typing import Tuple

import numpy as np

from lap import _hip

# ret codes of lapwarm_oracle_duals (include/lapwarm_hip.h)
_NEGATIVE_CYCLE, _INFEASIBLE, _SLACKNESS, _NOT_PERMUTATION, _NON_FINITE = 1, 2, 3, 4, 5


def _prepare(C, row_ind, col_ind):
    C = np.ascontiguousarray(np.asarray(C, dtype=float), dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1]:
        raise ValueError(f"square cost matrix expected, got shape {C.shape}")
    assert len(row_ind) == len(col_ind)
    n = C.shape[0]
    if n == 0:
        raise ValueError("empty cost matrix")
    if len(row_ind) != n:
        raise ValueError(f"a full matching of {n} pairs is expected, got {len(row_ind)}")
    rows = np.ascontiguousarray(np.asarray(row_ind), dtype=np.int32)
    cols = np.ascontiguousarray(np.asarray(col_ind), dtype=np.int32)
    return C, rows, cols


def _oracle_uv(C, rows, cols, tol=1e-12):
    """(u, v) of the reference's reconstruction on the device; raises as the reference does."""
    n = C.shape[0]
    u = np.empty(n, dtype=np.float64)
    v = np.empty(n, dtype=np.float64)
    lib = _hip.require_device()
    rc = lib.lapwarm_oracle_duals(C.ctypes.data_as(_hip.c_dp), n, rows.ctypes.data_as(_hip.c_ip),
                                  cols.ctypes.data_as(_hip.c_ip), u.ctypes.data_as(_hip.c_dp),
                                  v.ctypes.data_as(_hip.c_dp), float(tol))
    _hip.check(rc, "oracle_duals")
    if rc == 0:
        return u, v
    if rc == _NEGATIVE_CYCLE:
        raise RuntimeError("Negative cycle while solving difference constraints for v.")
    if rc == _INFEASIBLE:
        raise AssertionError("Dual infeasible after reconstruction (negative reduced costs).")
    if rc == _SLACKNESS:
        raise AssertionError("Complementary slackness violated on a matched edge.")
    if rc == _NOT_PERMUTATION:
        raise ValueError("row_ind / col_ind must each be a permutation of range(n)")
    if rc == _NON_FINITE:
        raise ValueError("cost matrix has non-finite entries")
    raise RuntimeError(f"lapwarm_oracle_duals failed (code {rc}): {_hip.last_error()}")


def dual_from_matching_diff_constraints(C, row_ind, col_ind, tol=1e-12):
    """Optimal duals (u, v) and the reduced-cost matrix (C - u) - v from a full matching."""
    C, rows, cols = _prepare(C, row_ind, col_ind)
    u, v = _oracle_uv(C, rows, cols, tol)
    from .advanced_dual import reduce_costs
    red = reduce_costs(C, u, v, shift_nonneg=False)
    return u, v, red


def _matching(C):
    import lap
    _, x, _ = lap.lapjv(C)
    return np.arange(C.shape[0], dtype=np.int32), np.ascontiguousarray(x, dtype=np.int32)


def _colmin(C):
    n = C.shape[0]
    out = np.empty(n, dtype=np.float64)
    lib = _hip.require_device()
    rc = lib.lapwarm_min_trick(C.ctypes.data_as(_hip.c_dp), n, None, out.ctypes.data_as(_hip.c_dp))
    if _hip.check(rc, "min_trick") != 0:
        raise RuntimeError(f"min_trick failed (code {rc})")
    return out


def compute_oracle_duals(C: np.ndarray, noise_level: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """Oracle duals of C from its optimal matching, with optional Gaussian noise (np.random.seed(42))."""
    C = np.ascontiguousarray(np.asarray(C, dtype=float), dtype=np.float64)
    n = C.shape[0]
    rows, cols = _matching(C)
    try:
        u_star, v_star = _oracle_uv(*_prepare(C, rows, cols))
    except (RuntimeError, AssertionError) as e:
        print(f"Warning: Difference constraints failed ({e}), using fallback method")
        u_star = np.zeros(n, dtype=np.float64)
        v_star = _colmin(C)
        for r, c in zip(rows, cols):
            u_star[r] = C[r, c] - v_star[c]

    if noise_level > 0:
        np.random.seed(42)
        u_noise = np.random.normal(0, noise_level, n)
        v_noise = np.random.normal(0, noise_level, n)
        u_star += u_noise
        v_star += v_noise

    return u_star.astype(np.float64), v_star.astype(np.float64)
