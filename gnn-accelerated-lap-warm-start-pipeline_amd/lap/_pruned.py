"""Exact dense lapjv through sparse LAPMOD on the device (gnn.pipeline.WarmStartPipeline.lapjv_pruned_ragged over
csrc/prune_price.hip and lapwarm_lapmod_ragged).

    lapjv_pruned(cost, k=16, v=None, return_cost=True)        -> (opt, x, y) or (x, y)   int32
    lapjv_pruned_many(costs, k=16, v=None, return_cost=True)  -> [(opt, x, y), ...]

Every row keeps its diagonal and its k cheapest columns (cheapest after subtracting the optional column seed `v`);
LAPMOD solves that graph, its duals price the absent entries, and rows gain entries until none prices in: the sparse
optimum is then the dense one.  An instance that is not certified within 32 rounds, or whose costs LAPMOD refuses
(outside [0, 1e6), inf, NaN), is solved by the dense lapjv instead, so the result is always an optimum.  Like
`lapjv_extended` the names are importable from `lap` without being listed in `__all__`.  Every argument error is
raised before any device work.
"""
from __future__ import annotations

import numpy as np

from . import _hip


def _check(costs, k, seeds):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("Argument 'k' must be an int, not %s" % type(k).__name__)
    if not 1 <= k <= 256:
        raise ValueError('k must be in 1..256, not %d' % k)
    mats = [np.asarray(c, dtype=np.float64) for c in costs]
    if seeds is not None and len(seeds) != len(mats):
        raise ValueError('one seed per cost matrix expected: %d for %d' % (len(seeds), len(mats)))
    out = []
    for b, c in enumerate(mats):
        if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
            raise ValueError('Square cost array expected, not %s' % (tuple(c.shape),))
        s = None
        if seeds is not None and seeds[b] is not None:
            s = np.asarray(seeds[b], dtype=np.float64)
            if s.shape != (c.shape[0],):
                raise ValueError('the seed of an n x n matrix must have length n: %s for n = %d'
                                 % (tuple(s.shape), c.shape[0]))
            if not np.all(np.isfinite(s)):
                raise ValueError('the seed must be finite')
        out.append(s)
    return mats, int(k), out


def _solve(mats, k, seeds):
    _hip.require_device()
    import torch
    from gnn.features import ragged_pack
    from gnn.pipeline import shared_pipeline
    pipe = shared_pipeline()
    pack = ragged_pack(mats, pipe.device)
    seed = None
    if any(s is not None for s in seeds):
        host = np.zeros((len(mats), pack.N), dtype=np.float64)
        for b, s in enumerate(seeds):
            if s is not None:
                host[b, :s.size] = s
        seed = torch.from_numpy(host).to(pipe.device)
    res = pipe._pruned_packed(pack, k, seed)
    return [(float(r["cost"]), r["x"].cpu().numpy(), r["y"].cpu().numpy()) for r in res]


def lapjv_pruned(cost, k=16, v=None, return_cost=True):
    """The optimum of a square dense cost matrix through the pruned route: ``(opt, x, y)`` or ``(x, y)``, int32.
    `v`: an optional finite column seed of length n (a predicted dual); it decides which entries round 0 keeps."""
    mats, k, seeds = _check([cost], k, None if v is None else [v])
    opt, x, y = _solve(mats, k, seeds)[0]
    return (opt, x, y) if return_cost else (x, y)


def lapjv_pruned_many(costs, k=16, v=None, return_cost=True):
    """``lapjv_pruned`` of every matrix of ``costs`` in one ragged device solve; `v` a sequence of seeds (None for
    an instance without one) or None."""
    if costs is None:
        raise TypeError("Argument 'costs' must not be None")
    costs = list(costs)
    mats, k, seeds = _check(costs, k, None if v is None else list(v))
    if not mats:
        return []
    return [(opt, x, y) if return_cost else (x, y) for opt, x, y in _solve(mats, k, seeds)]
