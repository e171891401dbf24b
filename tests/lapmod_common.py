"""Reader of tests/golden/lapmod_cases.npz and lapmod_long_rows.npz (written by tests/golden/make_lapmod.py), shared
by the lapmod tests."""
from functools import lru_cache

import numpy as np

from conftest import GOLDEN

FP_VERSIONS = (1, 2, 3)
FILES = ("lapmod_cases.npz", "lapmod_long_rows.npz")
EXTRAS = ("arr_first_above", "arr_first_far")  # of dec_single193: make_lapmod.arr_first_values


@lru_cache(maxsize=1)
def load_cases():
    """label -> dict(n, cc fp64, ii, kk int32, solvable, strict, aug, dyn, ref {fp: (ret, x, y)}, v {fp: the
    reference's final column duals; solvable cases only, FP_DYNAMIC under the search it selects}), the cases of
    the second file behind those of the first."""
    cases = {}
    for name in FILES:
        z = np.load(GOLDEN / name, allow_pickle=False)
        if "lds_max_n" in z.files:
            lds_max = int(z["lds_max_n"])
        for label in (str(s) for s in z["labels"]):
            g = lambda key: z[f"{label}__{key}"]  # noqa: E731
            c = dict(n=int(g("n")), cc=g("cc").astype(np.float64) / float(g("ccscale")),
                     ii=g("ii").astype(np.int32), kk=g("kk").astype(np.int32), solvable=bool(g("solvable")),
                     strict=bool(g("strict")), aug=bool(g("aug")), dyn=int(g("dyn")), ref={}, v={})
            for fp in FP_VERSIONS:
                if f"{label}__ret_{fp}" in z.files:
                    c["ref"][fp] = (int(g(f"ret_{fp}")), g(f"x_{fp}").astype(np.int32), g(f"y_{fp}").astype(np.int32))
                src = c["dyn"] if fp == 3 else fp
                if f"{label}__v_{src}" in z.files:
                    c["v"][fp] = g(f"v_{src}")
            for key in EXTRAS:
                if f"{label}__{key}" in z.files:
                    c[key] = int(g(key))
            assert label not in cases, label
            cases[label] = c
    return cases, lds_max


@lru_cache(maxsize=1)
def long_row_labels():
    """The labels of lapmod_long_rows.npz, in its order."""
    return tuple(str(s) for s in np.load(GOLDEN / FILES[1], allow_pickle=False)["labels"])


def problem(c):
    return c["n"], c["cc"], c["ii"], c["kk"]


def densify(c, absent=np.inf):
    n = c["n"]
    D = np.full((n, n), absent, dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(c["ii"]))
    D[rows, c["kk"]] = c["cc"]
    return D
