"""`LAPMODSolver`: the harness-facing object for the sparse solver, over `lap.lapmod_sparse` on the MI355X
(csrc/lapmod_sparse.hip).

What it must keep from the reference's wrapper (solvers/lapmod_solver.py:16-78): the `.name` string, the return
convention (arange(n), x as int64, cost as float), and how a dense matrix reaches the sparse solver:

  * every element becomes a CSR entry; with a `mask`, the elements it excludes and the non-finite ones are
    entered as lap.LARGE instead of being left out;
  * lapmod takes costs below 1e6 only, so a matrix whose largest finite element reaches 1e6 (always the case with
    a mask, because of the LARGE entries) is multiplied by 999999 / that element, and the cost divided by the
    same factor afterwards.
"""
from __future__ import annotations

import numpy as np

import lap
from lap._lapmod import lapmod_sparse, sparse_from_dense

from .lap_solver import _HostSolver, _f64

_COST_CEILING = 1000000   # lapmod's check_cost refuses this value and anything above it
_SCALED_PEAK = 999999.0   # what the largest finite element becomes


def _admissible_costs(C, mask):
    """A copy of C with lap.LARGE wherever `mask` (if given) excludes the element or the element is not finite."""
    costs = C.copy()
    if mask is not None:
        keep = np.asarray(mask, dtype=bool) & np.isfinite(C)
        costs[~keep] = lap.LARGE
    return costs


def _shrink_factor(costs):
    """1.0, or the factor that brings the largest finite element down to 999999."""
    peak = costs[np.isfinite(costs)].max()
    return _SCALED_PEAK / peak if peak >= _COST_CEILING else 1.0


class LAPMODSolver(_HostSolver):
    """Sparse Jonker-Volgenant (`lap.lapmod_sparse`) on the device, fed from a dense matrix."""

    name = "LAPMOD"

    def __init__(self):
        self.name = type(self).name

    def solve(self, C, mask=None, fp_version=lap.FP_DYNAMIC):
        C = _f64(C)
        costs = _admissible_costs(C, mask)
        factor = _shrink_factor(costs)
        if factor != 1.0:
            costs = costs * factor
        cost, x, _ = lapmod_sparse(*sparse_from_dense(costs), fp_version=fp_version)
        if factor != 1.0:
            cost = cost / factor
        return np.arange(C.shape[0], dtype=np.int64), np.asarray(x, dtype=np.int64), float(cost)
