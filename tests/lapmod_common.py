"""Reader of tests/golden/lapmod_cases.npz (written by tests/golden/make_lapmod.py), shared by the lapmod tests."""
from functools import lru_cache

import numpy as np

from conftest import GOLDEN

FP_VERSIONS = (1, 2, 3)


@lru_cache(maxsize=1)
def load_cases():
    """label -> dict(n, cc fp64, ii, kk int32, solvable, strict, aug, dyn, ref {fp: (ret, x, y)}, v {fp: the
    reference's final column duals; solvable cases only, FP_DYNAMIC under the search it selects})."""
    z = np.load(GOLDEN / "lapmod_cases.npz", allow_pickle=False)
    cases = {}
    for label in (str(s) for s in z["labels"]):
        g = lambda key: z[f"{label}__{key}"]  # noqa: E731
        c = dict(n=int(g("n")), cc=g("cc").astype(np.float64) / float(g("ccscale")), ii=g("ii").astype(np.int32),
                 kk=g("kk").astype(np.int32), solvable=bool(g("solvable")), strict=bool(g("strict")),
                 aug=bool(g("aug")), dyn=int(g("dyn")), ref={}, v={})
        for fp in FP_VERSIONS:
            if f"{label}__ret_{fp}" in z.files:
                c["ref"][fp] = (int(g(f"ret_{fp}")), g(f"x_{fp}").astype(np.int32), g(f"y_{fp}").astype(np.int32))
            src = c["dyn"] if fp == 3 else fp
            if f"{label}__v_{src}" in z.files:
                c["v"][fp] = g(f"v_{src}")
        cases[label] = c
    return cases, int(z["lds_max_n"])


def problem(c):
    return c["n"], c["cc"], c["ii"], c["kk"]


def densify(c, absent=np.inf):
    n = c["n"]
    D = np.full((n, n), absent, dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(c["ii"]))
    D[rows, c["kk"]] = c["cc"]
    return D
