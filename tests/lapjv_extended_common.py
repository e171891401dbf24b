"""Reader of tests/golden/lapjv_extended_cases.npz and a NumPy restatement of what the reference's
`lapjv` does around `lapjv_internal` for `extend_cost` / `cost_limit` (LAP/_lapjv_cpp/_lapjv.pyx:77-95
and :115-124).  Shared by test_lapjv_extended_host.py, test_gpu_lapjv_extended.py and the generator
tests/golden/make_lapjv_extended.py."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "lapjv_extended_cases.npz"


def extended_n(n_rows, n_cols, extend_cost, cost_limit):
    if cost_limit < np.inf:
        return n_rows + n_cols
    return max(n_rows, n_cols) if extend_cost else n_rows


def build_E(cost, extend_cost, cost_limit):
    """_lapjv.pyx:84-95, statement by statement."""
    cost_c = np.ascontiguousarray(cost, dtype=np.double)
    n_rows, n_cols = cost_c.shape
    if cost_limit < np.inf:
        n = n_rows + n_cols
        E = np.empty((n, n), dtype=np.double)
        E[:] = cost_limit / 2.
        E[n_rows:, n_cols:] = 0
        E[:n_rows, :n_cols] = cost_c
        return E
    if extend_cost:
        n = max(n_rows, n_cols)
        E = np.zeros((n, n), dtype=np.double)
        E[:n_rows, :n_cols] = cost_c
        return E
    return cost_c


def finish(E, x, y, n_rows, n_cols):
    """_lapjv.pyx:116-122 on the solver's x, y of the n x n problem: (opt, x, y)."""
    x_c = np.array(x, dtype=np.int32)
    y_c = np.array(y, dtype=np.int32)
    x_c[x_c >= n_cols] = -1
    y_c[y_c >= n_rows] = -1
    x_c = x_c[:n_rows]
    y_c = y_c[:n_cols]
    opt = E[np.nonzero(x_c != -1)[0], x_c[x_c != -1]].sum()
    return opt, x_c, y_c


def solve_with(dense_raw, cost, extend_cost, cost_limit):
    """The reference's lapjv for an extended / limited problem with `dense_raw(E) -> (ret, x, y, ...)` as
    lapjv_internal.  Returns (opt, x, y, rest) where rest is whatever dense_raw returns after y."""
    n_rows, n_cols = np.shape(cost)
    E = build_E(cost, extend_cost, cost_limit)
    out = dense_raw(E)
    assert out[0] == 0, out[0]
    return finish(E, out[1], out[2], n_rows, n_cols) + (out[3:],)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


class ExtendedCases:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path, allow_pickle=False)
        self.meta = json.loads(str(self.z["meta"]))

    def __len__(self):
        return len(self.meta)

    @property
    def labels(self):
        return [m["label"] for m in self.meta]

    def case(self, k):
        """label, C, extend_cost, cost_limit, opt, x, y, and y_alt (a second accepted y) or None."""
        m = dict(self.meta[k])
        z = self.z
        m["C"] = np.ascontiguousarray(z[f"c{k}_C"], dtype=np.float64)
        m["cost_limit"] = float(z[f"c{k}_limit"])
        m["opt"] = float(z[f"c{k}_opt"])
        m["x"] = z[f"c{k}_x"]
        m["y"] = z[f"c{k}_y"]
        m["y_alt"] = z[f"c{k}_y_alt"] if f"c{k}_y_alt" in z.files else None
        return m


def assert_case(c, opt, x, y):
    """x, y, opt equal the reference's, bit for bit.  Where the reference's own test accepts a second y
    (test_arr_loop.py:59-60) that one passes too, with the x that belongs to it and the optimum to the
    1e-10 the reference's test asks."""
    label = c["label"]
    assert x.dtype == np.int32 and y.dtype == np.int32, label
    if c["y_alt"] is not None and np.array_equal(y, c["y_alt"]) and not np.array_equal(y, c["y"]):
        rows = np.nonzero(x != -1)[0]
        assert np.array_equal(y[x[rows]], rows) and len(rows) == (y != -1).sum(), (label, x, y)
        assert abs(opt - c["opt"]) <= 1e-10 * abs(c["opt"]), (label, opt, c["opt"])
        return
    assert np.array_equal(x, c["x"]), (label, x, c["x"])
    assert np.array_equal(y, c["y"]), (label, y, c["y"])
    assert bits(opt) == bits(c["opt"]), (label, opt, c["opt"])
