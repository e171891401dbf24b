#!/usr/bin/env python3
"""Generate tests/golden/lapjv_extended_cases.npz FROM THE REFERENCE.

Runs only where the reference build oracle/_ref/liblap_ref.so exists (the reference's own lapjv.cpp,
compiled unmodified).  For every case the square matrix E is built by numpy exactly as
LAP/_lapjv_cpp/_lapjv.pyx:84-95 does, `lapjv_internal` of the reference build solves it, and
_lapjv.pyx:116-122 is applied to its x, y (tests/lapjv_extended_common.py restates both steps).  Stored
as data: the cost matrix, extend_cost, cost_limit, and the resulting opt, x, y.

The three known answers of the reference's own tests go in too, and are asserted here:
LAP/lap/tests/test_lapjv.py:34-39 (extension), :52-57 (cost limit), test_arr_loop.py:45-60.

Usage:  python tests/golden/make_lapjv_extended.py          (from the repo root)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from lapjv_extended_common import GOLDEN, solve_with  # noqa: E402
from oracle import ref  # noqa: E402

cases = []
arrays = {}


def add(label, C, extend_cost, cost_limit, y_alt=None):
    k = len(cases)
    C = np.ascontiguousarray(C, dtype=np.float64)
    opt, x, y, _ = solve_with(ref.dense_raw, C, extend_cost, cost_limit)
    cases.append(dict(label=label, extend_cost=bool(extend_cost), n_rows=int(C.shape[0]), n_cols=int(C.shape[1])))
    arrays[f"c{k}_C"] = C
    arrays[f"c{k}_limit"] = np.float64(cost_limit)
    arrays[f"c{k}_opt"] = np.float64(opt)
    arrays[f"c{k}_x"] = x
    arrays[f"c{k}_y"] = y
    if y_alt is not None:
        arrays[f"c{k}_y_alt"] = np.asarray(y_alt, dtype=np.int32)
    print(f"{label:34s} {C.shape[0]:3d} x {C.shape[1]:3d}  matched {(x != -1).sum():3d}  opt {opt!r}", flush=True)
    return opt, x, y


# ---- 1. the reference's known answers
# get_dense_8x8_int (LAP/lap/tests/test_utils.py), the matrix of test_lapjv.py's small cases
D8 = np.array([[1000, 2, 11, 10, 8, 7, 6, 5], [6, 1000, 1, 8, 8, 4, 6, 7], [5, 12, 1000, 11, 8, 12, 3, 11],
               [11, 9, 10, 1000, 1, 9, 8, 10], [11, 11, 9, 4, 1000, 2, 10, 9], [12, 8, 5, 2, 11, 1000, 11, 9],
               [10, 11, 12, 10, 9, 12, 1000, 3], [10, 10, 10, 10, 6, 3, 1, 1000]], dtype=np.float64)
opt, x, y = add("known_extension_2x4", D8[:2, :4], True, np.inf)
assert opt == 3.0 and list(x) == [1, 2] and list(y) == [-1, 0, 1, -1]
opt, x, y = add("known_cost_limit_3x3", D8[:3, :3], False, 4.99)
assert opt == 3.0 and list(x) == [1, 2, -1] and list(y) == [-1, 0, 1]
cc = np.array([2.593883482138951146e-01, 3.080381437461217620e-01, 1.976243020727339317e-01,
               2.462740976049606068e-01, 4.203993396282833528e-01, 4.286184525458427985e-01,
               1.706431415909629434e-01, 2.192929371231896185e-01, 2.117769622802734286e-01,
               2.604267578125001315e-01])
ii = np.array([0, 0, 1, 1, 2, 2, 5, 5, 6, 6])
jj = np.array([0, 1, 0, 1, 1, 2, 0, 1, 0, 1])
A = np.empty((7, 3))
A[:] = 1000.
A[ii, jj] = cc
opt, x, y = solve_with(ref.dense_raw, A, True, np.inf)[:3]
assert abs(opt - 0.8455356917416) <= 1e-10 * 0.8455356917416
both = ([5, 1, 2], [1, 5, 2])
assert list(y) in both
add("known_arr_loop_7x3", A, True, np.inf, y_alt=both[1 - both.index(list(y))])


# ---- 2. shapes x cost kinds x limits
def uniform(rs, shape):
    return rs.uniform(size=shape)


def ties(rs, shape):
    return rs.randint(1, 10, size=shape).astype(np.float64)


def limits_for(C):
    """below every entry; at the median of the row minima (about half of the rows have an entry below it;
    between two integers for the integer costs); at the lower quartile and the middle of the range;
    above every entry"""
    lo, hi = C.min(), C.max()
    tight = float(np.median(C.min(axis=1))) + (0.5 if np.all(C == np.round(C)) else 0.0)
    return (("below", lo * 0.5), ("tight", tight), ("q25", float(np.quantile(C, 0.25))),
            ("mid", float((lo + hi) / 2.)), ("above", hi * 2.5 + 1.0))


SHAPES = (("tall", (37, 12)), ("wide", (13, 40)), ("square", (24, 24)), ("one_row", (1, 9)),
          ("one_col", (11, 1)), ("big", (40, 60)), ("odd", (15, 7)))
rs = np.random.RandomState(20240607)
for sname, shape in SHAPES:
    for kname, kind in (("uniform", uniform), ("ties", ties)):
        C = kind(rs, shape)
        add(f"{sname}_{kname}_extend", C, True, np.inf)
        for lname, lim in limits_for(C):
            if sname in ("big", "odd") and lname in ("below", "above"):
                continue
            # extend_cost does not change a limited problem (_lapjv.pyx:84-90); pass it on the
            # rectangular shapes, where the reference demands it
            add(f"{sname}_{kname}_limit_{lname}", C, shape[0] != shape[1], lim)
# a square matrix: limited without extend_cost above; extended without a limit; both
C = uniform(rs, (16, 16))
add("square16_extend_only", C, True, np.inf)
add("square16_limit_and_extend", C, True, 0.3)
add("one_by_one_limit_above", np.array([[2.5]]), False, 10.0)
add("one_by_one_limit_below", np.array([[2.5]]), False, 1.0)
add("one_by_one_extend", np.array([[2.5]]), True, np.inf)

arrays["meta"] = np.array(json.dumps(cases))
np.savez_compressed(GOLDEN, **arrays)
print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes, {len(cases)} cases)")
