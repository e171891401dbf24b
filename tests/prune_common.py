"""The pruned exact solve (dense LAP through sparse LAPMOD) restated in NumPy, its case list, and the reader of
tests/golden/prune_cases.npz (written by tests/golden/make_prune.py).  Shared by the prune tests.

The contract, per instance ("Exact dense LAP through sparse LAPMOD"): round 0 keeps, per row, the
diagonal and the k columns with the smallest key C_ij - s_j (C_ij without a seed), ties to the lower column; LAPMOD
solves the CSR; pricing adds to row i the at most m = k absent columns with the smallest C_ij - v_j among those
below u_i = C[i][x_i] - v[x_i]; no such column anywhere certifies the solve."""
from functools import lru_cache

import numpy as np

from conftest import GOLDEN

LARGE = 1e6
FAMILIES = ("uniform", "integer", "metric", "lowrank", "constant")


# ------------------------------------------------------------------------------------------- the restatement
def grow(C, rows, key_vector, bound, m):
    """One grow step.  `rows`: the current columns of every row (sorted int arrays); `key_vector` [n] or None;
    `bound` [n] or None (+inf).  Returns (new rows, viol): row i gains the min(m, |E_i|) members of
    E_i = {j absent from row i: C_ij - key_j < bound_i} with the smallest key, ties to the lower column."""
    n = C.shape[0]
    out, viol = [], 0
    for i in range(n):
        key = C[i] - key_vector if key_vector is not None else C[i]
        elig = key < (np.inf if bound is None else bound[i])
        elig[rows[i]] = False
        cand = np.flatnonzero(elig)
        viol += cand.size
        order = np.lexsort((cand, key[cand]))  # by key, then by column
        out.append(np.sort(np.concatenate((np.asarray(rows[i], dtype=np.int64), cand[order[:m]]))))
    return out, viol


def to_csr(C, rows):
    """(cc fp64, ii int32, kk int32) of the rows, values read from C."""
    ii = np.zeros(len(rows) + 1, dtype=np.int32)
    ii[1:] = np.cumsum([len(r) for r in rows])
    kk = np.concatenate(rows).astype(np.int32)
    cc = np.concatenate([C[i, r] for i, r in enumerate(rows)]).astype(np.float64)
    return cc, ii, kk


def admissible(C, seed=None):
    C = np.asarray(C, dtype=np.float64)
    ok = bool(np.all(np.isfinite(C)) and np.all(C >= 0.0) and np.all(C < LARGE))
    return ok and (seed is None or bool(np.all(np.isfinite(seed))))


def serial_cost(C, x):
    total = 0.0
    for i in range(C.shape[0]):
        total = total + C[i, x[i]]
    return total


def solve_pruned(C, k, lapmod, seed=None, max_rounds=32):
    """The whole loop; `lapmod(n, cc, ii, kk) -> (x, v)` is the sparse solve (FP_DYNAMIC).  Returns a dict: ret, x,
    u, v, cost, rounds, nnz, viol_last, trace = [(nnz, viol)] per solve and rows, the columns of the last CSR solved."""
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    if not admissible(C, seed):
        return dict(ret=3, x=np.full(n, -1), u=np.zeros(n), v=np.zeros(n), cost=np.inf, rounds=0, nnz=0,
                    viol_last=-1, trace=[])
    rows, _ = grow(C, [np.array([i]) for i in range(n)], seed, None, k)
    trace = []
    while True:
        cc, ii, kk = to_csr(C, rows)
        x, v = lapmod(n, cc, ii, kk)
        u = C[np.arange(n), x] - v[x]
        grown, viol = grow(C, rows, v, u, k)
        trace.append((int(ii[n]), int(viol)))
        if viol == 0 or len(trace) >= max_rounds:
            return dict(ret=0 if viol == 0 else 2, x=np.asarray(x, dtype=np.int32), u=u, v=v,
                        cost=serial_cost(C, x), rounds=len(trace), nnz=int(ii[n]), viol_last=int(viol), trace=trace,
                        rows=rows)
        rows = grown


# ------------------------------------------------------------------------------------------- the cases
def family_matrix(family, n, seed):
    """Deterministic from (family, n, seed)."""
    rng = np.random.default_rng([FAMILIES.index(family), n, seed])
    if family == "uniform":
        return rng.random((n, n))
    if family == "integer":
        return rng.integers(1, 101, size=(n, n)).astype(np.float64)
    if family == "metric":
        p, q = rng.random((n, 2)), rng.random((n, 2))
        return np.sqrt(((p[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))
    if family == "lowrank":
        r = 3
        return rng.random((n, r)) @ rng.random((r, n)) + 0.01 * rng.random((n, n))
    if family == "constant":
        return np.full((n, n), 7.0)
    raise ValueError(family)


# (label, family, n, k, seed): sizes 1..600, every family, k from 1 to 256
CASES = (
    ("uniform_n1_k16", "uniform", 1, 16, 1),
    ("integer_n2_k1", "integer", 2, 1, 2),
    ("uniform_n17_k16", "uniform", 17, 16, 3),   # n - 1 <= k: every column is kept
    ("constant_n33_k4", "constant", 33, 4, 4),
    ("metric_n63_k4", "metric", 63, 4, 5),
    ("integer_n64_k16", "integer", 64, 16, 6),
    ("lowrank_n65_k4", "lowrank", 65, 4, 7),
    ("uniform_n65_k1", "uniform", 65, 1, 8),
    ("constant_n65_k64", "constant", 65, 64, 9),
    ("metric_n257_k16", "metric", 257, 16, 10),
    ("integer_n257_k4", "integer", 257, 4, 11),
    ("lowrank_n257_k64", "lowrank", 257, 64, 12),
    ("uniform_n300_k256", "uniform", 300, 256, 13),
    ("uniform_n600_k16", "uniform", 600, 16, 14),
    ("integer_n600_k16", "integer", 600, 16, 15),
    ("metric_n400_k16", "metric", 400, 16, 16),
    ("lowrank_n200_k16", "lowrank", 200, 16, 17),
    ("constant_n129_k16", "constant", 129, 16, 18),
    ("lowrank_n90_k16", "lowrank", 90, 16, 19),
)


def case_matrix(label):
    _, family, n, _, seed = next(c for c in CASES if c[0] == label)
    return family_matrix(family, n, seed)


@lru_cache(maxsize=1)
def load_fixture():
    """label -> dict(k, family, n, seed, trace [(nnz, viol)], x int32, v fp64, cost)."""
    z = np.load(GOLDEN / "prune_cases.npz", allow_pickle=False)
    out = {}
    for label in (str(s) for s in z["labels"]):
        g = lambda key: z[f"{label}__{key}"]  # noqa: E731
        out[label] = dict(k=int(g("k")), family=str(g("family")), n=int(g("n")), seed=int(g("seed")),
                          trace=[tuple(int(t) for t in row) for row in g("trace")],
                          x=g("x").astype(np.int32), v=g("v"), cost=float(g("cost")))
    return out


def reference_lapmod():
    """The sparse solve of the restatement by the reference's lapmod_v (FP_DYNAMIC), or None without oracle/_ref."""
    from oracle import ref
    try:
        lib = ref.lapmod_lib()
    except (FileNotFoundError, OSError):
        return None

    def lapmod(n, cc, ii, kk):
        cc = np.ascontiguousarray(cc, dtype=np.float64)
        ii = np.ascontiguousarray(ii, dtype=np.uint32)
        kk = np.ascontiguousarray(kk, dtype=np.uint32)
        x, y, v = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32), np.full(n, np.nan)
        ret = lib.lapmod_v(n, cc.ctypes.data, ii.ctypes.data, kk.ctypes.data, x.ctypes.data, y.ctypes.data,
                           v.ctypes.data, 3)
        assert ret == 0, ret
        return x, v
    return lapmod
