"""Sparse LAPMOD on the device: mirror of LAP/lap/lapmod.py:248-340 and _lapjv.pyx:134-158 over
lapwarm_lapmod_ragged (csrc/lapmod_sparse.hip).

    lapmod_sparse(n, cc, ii, kk, fast=True, return_cost=True, fp_version=FP_DYNAMIC) -> (opt, x, y) or (x, y)
    lapmod_many(problems, fp_version=FP_DYNAMIC, return_cost=True)                   -> [(opt, x, y), ...]
    get_cost, sparse_from_dense, sparse_from_masked                                  -- the reference's helpers

`lap.lapmod` itself still raises NotImplementedError and `lap.__all__` is unchanged: tests/test_host_logic.py
asserts both.  The names above are importable from `lap` without being listed, as `lapjv_extended` is.  Once
that assertion is retired, routing is three lines in lap/__init__.py: import `lapmod_sparse as lapmod` from this
module, delete the raising `lapmod`, and keep "lapmod" in `__all__`.

Differences from the reference, all documented in DESIGN.md: `fast=False` takes the same device path (and gives
the same result); NaN in `cc` raises ValueError (the reference lets it through); unsorted or out-of-range `kk`,
a bad `ii` or an `fp_version` outside 1..3 raise ValueError; a problem without a perfect matching returns x, y all
-1 and cost inf where the reference reads uninitialised memory.
"""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from . import _hip
from ._lapjv import FP_1_, FP_2_, FP_DYNAMIC_, LARGE_

MAX_N = 65535  # the reference's 32-bit `current * n` and `n * n` wrap from 65536 on: not taken


def sparse_from_dense(cost):
    """(n, cc, ii, kk) with every element of a dense matrix as an entry."""
    cost = np.asarray(cost)
    n_rows, n_cols = cost.shape
    cc = cost.flatten()
    ii = np.arange(n_rows + 1, dtype=int) * n_cols
    kk = np.tile(np.arange(n_cols, dtype=int), n_rows)
    return n_rows, cc, ii, kk


def sparse_from_masked(cost, mask=None):
    """(n, cc, ii, kk) with the elements of `cost` where `mask` holds (default: the elements that are not inf)."""
    cost = np.asarray(cost)
    if mask is None:
        mask = np.logical_not(np.isinf(cost))
    mask = np.asarray(mask, dtype=bool)
    n_rows, n_cols = cost.shape
    cc = cost[mask].flatten()
    ii = np.zeros((n_rows + 1,), dtype=int)
    ii[1:] = np.cumsum(mask.sum(axis=1))
    kk = np.tile(np.arange(n_cols, dtype=int), n_rows)[mask.flatten()]
    return n_rows, cc, ii, kk


def get_cost(n, cc, ii, kk, x0):
    """Sum of cc over the entries (i, x0[i]), rows left to right; inf when an assigned column is absent from its
    row."""
    ret = 0
    for i, j in enumerate(x0):
        lo, hi = ii[i], ii[i + 1]
        k = bisect_left(kk[lo:hi], j)
        if k >= hi - lo or kk[lo + k] != j:
            return np.inf
        ret += cc[lo + k]
    return ret


# the reference's check_cost messages (LAP/lap/lapmod.py:248-259), in the order it raises them
_ZERO_ROWS = 'Cost matrix has zero rows.'
_ZERO_COLS = 'Cost matrix has zero columns.'
_NEGATIVE = 'Cost matrix values must be non-negative.'
_TOO_LARGE = 'Cost matrix values must be less than %s' % LARGE_


def _check_cost(n, cc, ii, kk):
    """The reference's four refusals, with its texts and in its order, and NaN (which it lets through)."""
    if n == 0:
        raise ValueError(_ZERO_ROWS)
    if len(kk) == 0:
        raise ValueError(_ZERO_COLS)
    values = np.asarray(cc, dtype=np.float64)
    if np.isnan(values).any():
        raise ValueError('Cost matrix values must not be NaN.')
    if np.any(values < 0):
        raise ValueError(_NEGATIVE)
    if np.any(values >= LARGE_):
        raise ValueError(_TOO_LARGE)


def _check_problem(n, cc, ii, kk, fp_version):
    """The reference's check_cost, then what the device solver relies on.  Returns contiguous fp64 / int32 copies."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError("Argument 'n' must be an int, not %s" % type(n).__name__)
    if n < 0:
        raise ValueError('n must be non-negative, not %d' % n)
    if n > MAX_N:
        raise ValueError('n must be at most %d, not %d' % (MAX_N, n))
    cc, ii, kk = np.asarray(cc), np.asarray(ii), np.asarray(kk)
    if cc.ndim != 1 or ii.ndim != 1 or kk.ndim != 1:
        raise ValueError('cc, ii and kk must be 1-dimensional')
    _check_cost(n, cc, ii, kk)
    if isinstance(fp_version, bool) or fp_version not in (FP_1_, FP_2_, FP_DYNAMIC_):
        raise ValueError('fp_version must be FP_1, FP_2 or FP_DYNAMIC (1, 2, 3), not %r' % (fp_version,))
    if len(ii) != n + 1 or ii[0] != 0 or ii[n] != len(cc) or len(cc) != len(kk) or np.any(np.diff(ii) < 0):
        raise ValueError('ii must hold n + 1 ascending row starts with ii[0] = 0 and ii[n] = len(cc) = len(kk)')
    if kk.min() < 0 or kk.max() >= n:
        raise ValueError('Column indices in kk must lie in 0..n-1.')
    unsorted = np.diff(kk) <= 0  # [k]: kk[k + 1] against kk[k]
    starts = np.asarray(ii[1:n], dtype=np.int64)
    unsorted[starts[(starts > 0) & (starts < len(kk))] - 1] = False  # a row's first entry follows another row
    if unsorted.any():
        raise ValueError('Column indices in kk must be sorted and unique within each row.')
    return (int(n), np.ascontiguousarray(cc, dtype=np.float64), np.ascontiguousarray(ii, dtype=np.int32),
            np.ascontiguousarray(kk, dtype=np.int32))


def _solve(problems, fp_version):
    """One upload and one device call; [(ret, x, y)] with x, y int32 of length n_b."""
    _hip.require_device()
    from gnn.pipeline import shared_pipeline, sparse_pack  # (torch is needed from here on only)
    pipe = shared_pipeline()
    out = pipe.lapmod_ragged(sparse_pack(problems, pipe.device), int(fp_version), want_stats=False)
    ret, x, y = out["ret"].cpu().numpy(), out["x"].cpu().numpy(), out["y"].cpu().numpy()
    res = []
    for b, (n, _, _, _) in enumerate(problems):
        if ret[b] not in (0, 1):
            raise RuntimeError('Unknown error (lapmod_internal returned %d).' % ret[b])
        res.append((int(ret[b]), x[b, :n].copy(), y[b, :n].copy()))
    return res


def lapmod_sparse(n, cc, ii, kk, fast=True, return_cost=True, fp_version=FP_DYNAMIC_):
    """The reference's ``lapmod``: Jonker-Volgenant on a square sparse (CSR) cost matrix, column indices sorted
    within each row.  Returns ``(opt, x, y)`` or ``(x, y)``, int32.  A problem without a perfect matching gives
    x, y all -1 and opt inf."""
    prob = _check_problem(n, cc, ii, kk, fp_version)
    _, x, y = _solve([prob], fp_version)[0]
    if return_cost:
        return get_cost(n, cc, ii, kk, x), x, y
    return x, y


def lapmod_many(problems, fp_version=FP_DYNAMIC_, return_cost=True):
    """``lapmod_sparse`` of every ``(n, cc, ii, kk)`` of ``problems`` with one upload and one device call: a list
    of ``(opt, x, y)`` or ``(x, y)``, each what ``lapmod_sparse`` returns for the problem alone.  Every argument
    error is raised before any device work."""
    if problems is None:
        raise TypeError("Argument 'problems' must not be None")
    raw = [tuple(p) for p in problems]
    for p in raw:
        if len(p) != 4:
            raise ValueError('every problem must be (n, cc, ii, kk)')
    probs = [_check_problem(n, cc, ii, kk, fp_version) for n, cc, ii, kk in raw]
    if not probs:
        return []
    out = []
    for (n, cc, ii, kk), (_, x, y) in zip(raw, _solve(probs, fp_version)):
        out.append((get_cost(n, cc, ii, kk, x), x, y) if return_cost else (x, y))
    return out
