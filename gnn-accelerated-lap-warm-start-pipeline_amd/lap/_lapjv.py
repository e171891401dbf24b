"""lapjv: mirror of LAP/_lapjv_cpp/_lapjv.pyx:38-129 over the HIP C ABI.  `lapjv` is the square, unlimited
path; `lapjv_extended` is the whole function, rectangular (`extend_cost`) and thresholded (`cost_limit`)
problems included."""
from __future__ import annotations

import numpy as np

from . import _hip

LARGE_ = 1000000  # LAP/_lapjv_cpp/lapjv.h:4
FP_1_, FP_2_, FP_DYNAMIC_ = 1, 2, 3


def lapjv(cost, extend_cost=False, cost_limit=np.inf, return_cost=True):
    """Jonker-Volgenant on a dense square cost matrix: returns ``(opt, x, y)`` (int32 x, y)."""
    if cost is None:
        raise TypeError("Argument 'cost' must not be None")
    cost = np.asarray(cost)
    if cost.ndim != 2:
        raise ValueError("2-dimensional array expected")
    cost_c = np.ascontiguousarray(cost, dtype=np.double)
    n_rows, n_cols = cost_c.shape
    if n_rows != n_cols and not extend_cost:
        raise ValueError("Square cost array expected. If cost is intentionally "
                         "non-square, pass extend_cost=True.")
    if extend_cost or cost_limit < np.inf:
        raise NotImplementedError(
            "extend_cost / cost_limit (rectangular and thresholded problems, _lapjv.pyx:79-95) are not "
            "routed through lapjv yet: call lap.lapjv_extended with the same arguments")
    n = n_rows
    x = np.empty((n,), dtype=np.int32)
    y = np.empty((n,), dtype=np.int32)
    if n > 0:
        lib = _hip.require_device()
        ret = lib.lapwarm_lapjv_dense(cost_c.ctypes.data_as(_hip.c_dp), n, x.ctypes.data_as(_hip.c_ip),
                                      y.ctypes.data_as(_hip.c_ip))
        _hip.check(ret, "lapjv")
        if ret != 0:
            if ret == -1:
                raise MemoryError("Out of memory.")
            raise RuntimeError("Unknown error (lapjv_internal returned %d)." % ret)
    if return_cost:
        opt = cost_c[np.arange(n_rows), x].sum()
        return opt, x, y
    return x, y


def lapjv_extended(cost, extend_cost=False, cost_limit=np.inf, return_cost=True):
    """The reference's ``lapjv`` for every combination of its arguments (_lapjv.pyx:38-129): returns
    ``(opt, x, y)`` or ``(x, y)``, int32 ``x`` (n_rows) and ``y`` (n_cols) with -1 for unmatched rows and
    columns.  With ``cost_limit < inf`` the problem solved is (n_rows + n_cols) square, else with
    ``extend_cost`` max(n_rows, n_cols) square; only ``cost`` is copied to the device, the square matrix is
    built there.  ``opt`` sums ``cost[i, x[i]]`` over the matched rows in numpy's summation order."""
    if cost is None:
        raise TypeError("Argument 'cost' must not be None")
    try:  # `double cost_limit` is converted when the arguments are parsed; a str is a TypeError there
        cost_limit = float(cost_limit)
    except ValueError:
        raise TypeError("must be real number, not %s" % type(cost_limit).__name__) from None
    cost = np.asarray(cost)
    if cost.ndim != 2:
        raise ValueError("2-dimensional array expected")
    cost_c = np.ascontiguousarray(cost, dtype=np.double)
    n_rows, n_cols = cost_c.shape
    if n_rows != n_cols and not extend_cost:
        raise ValueError("Square cost array expected. If cost is intentionally "
                         "non-square, pass extend_cost=True.")
    if not (extend_cost or cost_limit < np.inf):
        return lapjv(cost_c, return_cost=return_cost)
    x = np.full((n_rows,), -1, dtype=np.int32)
    y = np.full((n_cols,), -1, dtype=np.int32)
    opt = np.float64(0.0)
    if n_rows > 0 and n_cols > 0:  # else nothing can be matched: every entry stays -1
        lib = _hip.require_device()
        opt_c = _hip.ct.c_double(np.nan)
        ret = lib.lapwarm_lapjv_extended(cost_c.ctypes.data_as(_hip.c_dp), n_rows, n_cols, int(bool(extend_cost)),
                                         cost_limit, x.ctypes.data_as(_hip.c_ip), y.ctypes.data_as(_hip.c_ip),
                                         _hip.ct.byref(opt_c))
        _hip.check(ret, "lapjv_extended")
        if ret != 0:
            if ret == -1:
                raise MemoryError("Out of memory.")
            raise RuntimeError("Unknown error (lapjv_internal returned %d)." % ret)
        opt = np.float64(opt_c.value)
    if return_cost:
        return opt, x, y
    return x, y


def lapjv_many(costs, extend_cost=False, cost_limit=np.inf, return_cost=True):
    """``lapjv_extended`` of every matrix of ``costs`` (a sequence of 2-D arrays of any shapes) with far fewer
    launches: returns a list of ``(opt, x, y)``, or of ``(x, y)``, with exactly the dtypes and values
    ``lapjv_extended(cost, extend_cost, cost_limit_b, return_cost)`` returns for each.  ``cost_limit`` is a scalar
    or one value per matrix.  The matrices whose extended size is in the ragged class (n_rows + n_cols, or
    max(n_rows, n_cols) without a limit, up to 511) are packed, copied to the device once and solved by one
    ragged call (gnn.WarmStartPipeline.lapjv_extended_many); larger ones go through the batched entry, once per
    distinct shape.  Every argument error of ``lapjv_extended`` is raised before any device work."""
    if costs is None:
        raise TypeError("Argument 'costs' must not be None")
    mats = []
    for cost in costs:
        if cost is None:
            raise TypeError("Argument 'cost' must not be None")
        cost = np.asarray(cost)
        if cost.ndim != 2:
            raise ValueError("2-dimensional array expected")
        mats.append(np.ascontiguousarray(cost, dtype=np.double))
    if np.ndim(cost_limit) == 0:
        limits = [cost_limit] * len(mats)
    else:
        limits = list(cost_limit)
        if len(limits) != len(mats):
            raise ValueError("%d cost matrices but %d cost limits" % (len(mats), len(limits)))
    for k, t in enumerate(limits):
        try:
            limits[k] = float(t)
        except ValueError:
            raise TypeError("must be real number, not %s" % type(t).__name__) from None
    for c in mats:
        if c.shape[0] != c.shape[1] and not extend_cost:
            raise ValueError("Square cost array expected. If cost is intentionally "
                             "non-square, pass extend_cost=True.")
    out = [None] * len(mats)
    work = []
    for b, c in enumerate(mats):
        if c.shape[0] == 0 or c.shape[1] == 0:  # nothing to match: lapjv_extended answers without a device
            out[b] = lapjv_extended(c, extend_cost, limits[b], return_cost)
        else:
            work.append(b)
    if work:
        _hip.require_device()
        from gnn.pipeline import shared_pipeline  # (torch is needed from here on only)
        _, parts = shared_pipeline()._extended_many_parts([mats[b] for b in work], extend_cost,
                                                          [limits[b] for b in work], want_stats=False)
        for members, rows, cols, o in parts:
            ret, opt = o["ret"].cpu().numpy(), o["opt"].cpu().numpy()
            x, y = o["x"].cpu().numpy(), o["y"].cpu().numpy()
            for k, m in enumerate(members):
                if ret[k] != 0:
                    raise RuntimeError("Unknown error (lapjv_internal returned %d)." % ret[k])
                xb, yb = x[k, :rows[k]].copy(), y[k, :cols[k]].copy()
                out[work[m]] = (np.float64(opt[k]), xb, yb) if return_cost else (xb, yb)
    return out
