"""Dual utilities of the hot path, on the GPU (reference: solvers/advanced_dual.py:14-113).

Each function keeps the reference's signature and semantics; the dense row/column sweeps run
as HIP kernels over the C ABI (lapwarm_project_feasible / lapwarm_reduce_costs /
lapwarm_oracle_duals).  `make_feasible_duals` takes its matching from `lap.lapjv` instead of
SciPy's linear_sum_assignment (see solvers/dual_computation.py)."""
from typing import Optional, Tuple

import numpy as np

from lap import _hip


def _mat(C):
    return np.ascontiguousarray(np.asarray(C, dtype=float), dtype=np.float64)


def project_feasible(C: np.ndarray, u: np.ndarray, v: np.ndarray,
                     max_rounds: int = 50, tol: float = 1e-12) -> Tuple[np.ndarray, np.ndarray]:
    """u <- min(u, rowmin(C - v)); v <- min(v, colmin(C - u)); until min(C-u-v) >= -tol."""
    C = _mat(C)
    u = np.array(u, dtype=np.float64).copy()
    v = np.array(v, dtype=np.float64).copy()
    n = C.shape[0]
    if n == 0:
        return u, v
    lib = _hip.require_device()
    rc = lib.lapwarm_project_feasible(C.ctypes.data_as(_hip.c_dp), n, u.ctypes.data_as(_hip.c_dp),
                                      v.ctypes.data_as(_hip.c_dp), max(1, int(max_rounds)), float(tol))
    if _hip.check(rc, "project_feasible") != 0:
        raise RuntimeError(f"project_feasible failed (code {rc})")
    return u, v


def _reduce(C, u, v, shift_nonneg, want_matrix=True):
    C = _mat(C)
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    n = C.shape[0]
    out = np.empty_like(C) if want_matrix else None
    mn = np.zeros(1)
    lib = _hip.require_device()
    rc = lib.lapwarm_reduce_costs(C.ctypes.data_as(_hip.c_dp), n, u.ctypes.data_as(_hip.c_dp),
                                  v.ctypes.data_as(_hip.c_dp), int(bool(shift_nonneg)),
                                  out.ctypes.data_as(_hip.c_dp) if want_matrix else None,
                                  mn.ctypes.data_as(_hip.c_dp))
    if _hip.check(rc, "reduce_costs") != 0:
        raise RuntimeError(f"reduce_costs failed (code {rc})")
    return out, float(mn[0])


def reduce_costs(C: np.ndarray, u: np.ndarray, v: np.ndarray, shift_nonneg: bool = True) -> np.ndarray:
    """C' = C - u 1^T - 1 v^T; with shift_nonneg, minus min(C') when that is negative."""
    if np.asarray(C).shape[0] == 0:
        return np.ascontiguousarray(np.asarray(C, dtype=np.float64))
    return _reduce(C, u, v, shift_nonneg)[0]


def check_dual_feasible(C: np.ndarray, u: np.ndarray, v: np.ndarray, tol: float = 1e-8) -> bool:
    """Raises AssertionError when some reduced cost is below -tol."""
    _, mn = _reduce(C, u, v, False, want_matrix=False)
    if mn < -tol:
        raise AssertionError(f"Dual infeasible: min reduced cost {mn:.3e} < -tol")
    return True


# ---- many instances of different sizes per call: one pack (one upload of the costs), one call of the ragged entry
def _square_costs(costs):
    mats = [_mat(c) for c in costs]
    if len(mats) < 1:
        raise ValueError("at least one cost matrix expected")
    for c in mats:
        if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
            raise ValueError(f"square, non-empty cost matrices expected, not {tuple(c.shape)}")
    return mats


def _many_args(costs, us, vs):
    """Argument errors of the *_many functions, raised before any device work: the costs, then u, then v."""
    mats = _square_costs(costs)
    sizes = [c.shape[0] for c in mats]
    duals = []
    for name, seq in (("us", us), ("vs", vs)):
        seq = [np.asarray(x, dtype=np.float64) for x in seq]
        if len(seq) != len(mats):
            raise ValueError(f"{len(mats)} instances but {len(seq)} vectors in {name}")
        for b, (x, n) in enumerate(zip(seq, sizes)):
            if tuple(x.shape) != (n,):
                raise ValueError(f"{name}[{b}] has shape {tuple(x.shape)} for an instance of size {n}")
        duals.append(seq)
    return mats, sizes, duals[0], duals[1]


def _pad_upload(vectors, sizes, N, device):
    import torch
    host = np.zeros((len(sizes), N), dtype=np.float64)
    for b, (x, n) in enumerate(zip(vectors, sizes)):
        host[b, :n] = x
    return torch.from_numpy(host).to(device)


def _upload_pack(mats, device):
    """One RaggedPack of host matrices.  Each matrix is uploaded from where it lies and the batch is packed on the
    device: packing 32 matrices of 512 x 512 on the host first costs more than the projection itself."""
    import torch
    from gnn.features import ragged_pack
    return ragged_pack([torch.from_numpy(c).to(device) for c in mats], device)


def _split(padded, sizes):
    host = padded.cpu().numpy()
    return [host[b, :n].copy() for b, n in enumerate(sizes)]


def _packed(costs, us, vs, pipeline):
    from gnn.pipeline import shared_pipeline
    mats, sizes, us, vs = _many_args(costs, us, vs)
    pipe = pipeline if pipeline is not None else shared_pipeline()
    pack = _upload_pack(mats, pipe.device)
    u = _pad_upload(us, sizes, pack.N, pipe.device)
    v = _pad_upload(vs, sizes, pack.N, pipe.device)
    return pipe, pack, sizes, u, v


def project_feasible_many(costs, us, vs, max_rounds: int = 50, tol: float = 1e-12, pipeline=None):
    """project_feasible of B instances of different sizes in one device call (WarmStartPipeline.
    project_feasible_ragged): costs, us, vs are sequences of B matrices and vectors.  Returns a list of (u, v),
    each bit for bit what project_feasible gives the instance alone.  `pipeline`: a WarmStartPipeline, or None
    for the one this process shares."""
    pipe, pack, sizes, u, v = _packed(costs, us, vs, pipeline)
    u, v, _, _, _ = pipe.project_feasible_ragged(pack, u, v, max_rounds, tol)
    return list(zip(_split(u, sizes), _split(v, sizes)))


def _reduce_many(costs, us, vs, shift_nonneg, want_matrix, pipeline):
    pipe, pack, sizes, u, v = _packed(costs, us, vs, pipeline)
    out, gmin, _ = pipe.reduce_costs_ragged(pack, u, v, shift_nonneg, want_matrix)
    mats = None
    if want_matrix:
        flat, off, mats = out.cpu().numpy(), 0, []
        for n in sizes:
            mats.append(flat[off:off + n * n].reshape(n, n).copy())
            off += n * n
    return mats, gmin.cpu().numpy()


def reduce_costs_many(costs, us, vs, shift_nonneg: bool = True, pipeline=None):
    """reduce_costs of B instances of different sizes in one device call: a list of B matrices."""
    return _reduce_many(costs, us, vs, shift_nonneg, True, pipeline)[0]


def check_dual_feasible_many(costs, us, vs, tol: float = 1e-8, pipeline=None) -> bool:
    """check_dual_feasible of B instances in one device call.  Raises the reference's AssertionError for the
    first instance whose minimum reduced cost is below -tol, and names it."""
    _, mins = _reduce_many(costs, us, vs, False, False, pipeline)
    for b, mn in enumerate(mins.tolist()):
        if mn < -tol:
            raise AssertionError(f"Dual infeasible: min reduced cost {mn:.3e} < -tol (instance {b})")
    return True


def check_dual_and_match(C: np.ndarray, u: np.ndarray, v: np.ndarray,
                         rows: np.ndarray, cols: np.ndarray, tol: float = 1e-8) -> bool:
    """Dual feasibility ((C - u) - v >= -tol everywhere) and |reduced cost| <= 1e-6 on the matching."""
    C = _mat(C)
    u = np.ascontiguousarray(u, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    if C.shape[0] == 0:
        mn = np.inf
    else:
        _, mn = _reduce(C, u, v, False, want_matrix=False)
    nan = bool(np.isnan(u).any() or np.isnan(v).any() or np.isnan(C).any())
    assert mn >= -tol and not nan, "Dual infeasible: some reduced costs < 0"
    rows = np.asarray(rows)
    cols = np.asarray(cols)
    red_m = (C[rows, cols] - u[rows]) - v[cols]
    assert np.all(np.abs(red_m) <= 1e-6), "Complementary slackness violated on matched edges"
    return True


def make_feasible_duals(C: np.ndarray, iters: int = 2, noise_std: float = 0.0,
                        project_rounds: int = 2, rng: Optional[np.random.Generator] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Oracle duals of C's optimal matching, optional noise, then project_feasible (>= 10 rounds)."""
    from .dual_computation import _matching, _oracle_uv, _prepare
    C = _mat(C)
    rows, cols = _matching(C)
    C, rows, cols = _prepare(C, rows, cols)
    u, v = _oracle_uv(C, rows, cols)

    if noise_std and noise_std > 0:
        rng = rng or np.random.default_rng(0)
        u = u + rng.normal(0.0, noise_std, size=u.shape)
        v = v + rng.normal(0.0, noise_std, size=v.shape)

    rounds = max(int(project_rounds), int(iters or 0))
    u, v = project_feasible(C, u, v, max_rounds=max(10, rounds), tol=1e-12)
    return u, v


__all__ = ["project_feasible", "reduce_costs", "check_dual_feasible", "check_dual_and_match", "make_feasible_duals",
           "project_feasible_many", "reduce_costs_many", "check_dual_feasible_many"]
