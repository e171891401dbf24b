"""Reader of tests/golden/oracle_duals_cases.npz and a NumPy restatement of the oracle duals
(shared by test_oracle_duals_fixtures.py and test_gpu_oracle_duals.py)."""
import hashlib
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "oracle_duals_cases.npz"


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_C(recipe):
    from solvers.generators import generate_family
    fam, n, seed = recipe
    if fam == "int100":
        return np.random.RandomState(seed).randint(1, 101, size=(n, n)).astype(np.float64)
    return generate_family(fam, n, seed)


class OracleCases:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path, allow_pickle=False)
        self.meta = json.loads(str(self.z["meta"]))

    def __len__(self):
        return len(self.meta)

    def case(self, k):
        m = dict(self.meta[k])
        z = self.z
        C = z[f"c{k}_C"] if f"c{k}_C" in z.files else make_C(m["recipe"])
        m["C"] = np.ascontiguousarray(C, dtype=np.float64)
        for key in ("rows", "cols", "u", "v"):
            if f"c{k}_{key}" in z.files:
                m[key] = z[f"c{k}_{key}"]
        return m

    def indices(self, kind):
        return [k for k, m in enumerate(self.meta) if m["kind"] == kind]


def jacobi(C, rows, cols, cap=None):
    """Synchronous sweeps of v_b <- v_b > fl(v_a + fl(C[r,b] - C[r,a])) ? that : v_b from v = 0.
    Returns (v, sweeps) -- the last sweep changes nothing -- or (v, -1) after `cap` sweeps."""
    n = C.shape[1]
    cap = n + 2 if cap is None else cap
    W = C[rows, :] - C[rows, cols][:, None]
    v = np.zeros(n)
    for s in range(1, cap + 1):
        cand = (v[cols][:, None] + W).min(axis=0)
        nv = np.where(v > cand, cand, v)
        if np.array_equal(nv, v):
            return v, s
        v = nv
    return v, -1


def oracle_from_v(C, rows, cols, v):
    """Steps 3 and 4 of the reference: u from the matched pairs, then the mean gauge."""
    u = np.full(C.shape[0], np.nan)
    u[rows] = C[rows, cols] - v[cols]
    shift = (np.mean(u) + np.mean(v)) / 2.0
    return u - shift, v + shift


def pairwise_sum(a):
    """numpy's pairwise summation order for a contiguous fp64 vector (what np.mean uses)."""
    n = len(a)
    if n < 8:
        r = -0.0
        for x in a:
            r = r + x
        return r
    if n <= 128:
        r = [a[q] for q in range(8)]
        i = 8
        while i < n - n % 8:
            for q in range(8):
                r[q] = r[q] + a[i + q]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[i]
            i += 1
        return res
    n2 = (n // 2) & ~7
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])
