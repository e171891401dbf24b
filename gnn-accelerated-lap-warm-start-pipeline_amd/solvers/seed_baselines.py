"""Classical dual seeds for warm-start experiments, on the GPU
(reference: solvers/seed_baselines.py:18-112).

`seed_row_col_minima` is the reference's construction sweep for sweep (row minima, min-trick,
project_feasible) and is bit-identical to it.  `seed_noisy_optimal` keeps the reference's recipe
(optimal duals + Gaussian noise + projection) but takes the optimal duals from the cold JV solve
on the device instead of SciPy + Bellman-Ford (solvers/advanced_dual.py:85-113): any optimal dual
pair is a valid starting point, so the seeds are equivalent in quality, not bit-identical.  The
reference's own oracle duals are `solvers.make_feasible_duals` / `compute_oracle_duals`
(csrc/oracle_duals.hip).  `seed_greedy_matching` is not provided: a greedy matching is almost never
optimal, and the reference's difference-constraint step raises on it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from lap import _hip
from .advanced_dual import _pad_upload, _split, _square_costs, _upload_pack, project_feasible


def _row_min(C: np.ndarray, v: Optional[np.ndarray] = None) -> np.ndarray:
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    out = np.empty(n, dtype=np.float64)
    lib = _hip.require_device()
    vv = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    rc = lib.lapwarm_row_min(C.ctypes.data_as(_hip.c_dp), n,
                             vv.ctypes.data_as(_hip.c_dp) if vv is not None else None,
                             out.ctypes.data_as(_hip.c_dp))
    if _hip.check(rc, "row_min") != 0:
        raise RuntimeError(f"row_min failed (code {rc})")
    return out


def _min_trick(C: np.ndarray, u: np.ndarray) -> np.ndarray:
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    uu = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty(n, dtype=np.float64)
    lib = _hip.require_device()
    rc = lib.lapwarm_min_trick(C.ctypes.data_as(_hip.c_dp), n, uu.ctypes.data_as(_hip.c_dp),
                               out.ctypes.data_as(_hip.c_dp))
    if _hip.check(rc, "min_trick") != 0:
        raise RuntimeError(f"min_trick failed (code {rc})")
    return out


def seed_row_col_minima(C: np.ndarray, *, project_rounds: int = 50):
    """u = row minima, v = min_i (C_ij - u_i), then project_feasible (seed_baselines.py:18-37)."""
    C = np.asarray(C, dtype=np.float64)
    u = _row_min(C)
    v = _min_trick(C, u)
    return project_feasible(C, u, v, max_rounds=project_rounds)


def seed_noisy_optimal(C: np.ndarray, *, noise_std: float = 0.05,
                       rng: Optional[np.random.Generator] = None, project_rounds: int = 75):
    """Optimal duals (from the device cold JV) + N(0, noise_std) noise, re-projected."""
    import torch
    from gnn.one_gnn import OneGNN
    from gnn.pipeline import WarmStartPipeline
    rng = rng or np.random.default_rng()
    C = np.ascontiguousarray(C, dtype=np.float64)
    pipe = WarmStartPipeline(OneGNN(21), "cuda:0")
    _, u, v, ret = pipe.optimal_duals_batch(torch.from_numpy(C).cuda().unsqueeze(0))
    torch.cuda.synchronize()
    if int(ret[0]) != 0:
        raise RuntimeError(f"cold JV failed (code {int(ret[0])})")
    u_opt, v_opt = u[0].cpu().numpy(), v[0].cpu().numpy()
    u_noisy = u_opt + rng.normal(0.0, noise_std, size=u_opt.shape)
    v_noisy = v_opt + rng.normal(0.0, noise_std, size=v_opt.shape)
    return project_feasible(C, u_noisy, v_noisy, max_rounds=project_rounds)


def seed_row_col_minima_many(costs, project_rounds: int = 50, pipeline=None):
    """seed_row_col_minima of B instances of different sizes: one upload, the three ragged device calls of
    WarmStartPipeline.seed_row_col_minima_ragged, one download.  Returns a list of (u, v), each bit for bit what
    seed_row_col_minima gives the instance alone."""
    from gnn.pipeline import shared_pipeline
    mats = _square_costs(costs)
    pipe = pipeline if pipeline is not None else shared_pipeline()
    u, v, _, _, _ = pipe.seed_row_col_minima_ragged(_upload_pack(mats, pipe.device), project_rounds)
    sizes = [c.shape[0] for c in mats]
    return list(zip(_split(u, sizes), _split(v, sizes)))


def seed_noisy_optimal_many(costs, noise_std: float = 0.05, rng: Optional[np.random.Generator] = None,
                            project_rounds: int = 75, pipeline=None):
    """seed_noisy_optimal of B instances of different sizes, by the reference's own recipe
    (seed_baselines.py:91-110): the oracle duals of the optimal matching by difference constraints
    (WarmStartPipeline.oracle_duals_many) projected as make_feasible_duals projects them (10 rounds), plus
    N(0, noise_std) noise drawn on the host from `rng` instance by instance, u then v -- the reference's draw
    order --, then the ragged projection.  Where the optimal matching is unique the result has the reference's
    bits.  `pipeline`: a WarmStartPipeline, or None for the one this process shares; none is built per call."""
    from gnn.pipeline import shared_pipeline
    mats = _square_costs(costs)
    noise_std = float(noise_std)
    rng = rng or np.random.default_rng()
    pipe = pipeline if pipeline is not None else shared_pipeline()
    sizes = [c.shape[0] for c in mats]
    pack = _upload_pack(mats, pipe.device)
    x = pipe._matching_packed(pack)
    u, v, ret, _ = pipe.oracle_duals_ragged(pack, x)
    bad = [b for b, r in enumerate(ret.tolist()) if r != 0]
    if bad:
        raise RuntimeError(f"seed_noisy_optimal_many: oracle duals of instance {bad[0]} (n = {sizes[bad[0]]}) "
                           f"failed with code {int(ret[bad[0]])}")
    u, v, _, _, _ = pipe.project_feasible_ragged(pack, u, v, max_rounds=10, tol=1e-12)
    us, vs = _split(u, sizes), _split(v, sizes)
    for b in range(len(sizes)):  # the reference's order of draws
        us[b] = us[b] + rng.normal(0.0, noise_std, size=us[b].shape)
        vs[b] = vs[b] + rng.normal(0.0, noise_std, size=vs[b].shape)
    u = _pad_upload(us, sizes, pack.N, pipe.device)
    v = _pad_upload(vs, sizes, pack.N, pipe.device)
    u, v, _, _, _ = pipe.project_feasible_ragged(pack, u, v, max_rounds=project_rounds, tol=1e-12)
    return list(zip(_split(u, sizes), _split(v, sizes)))


__all__ = ["seed_row_col_minima", "seed_noisy_optimal", "seed_row_col_minima_many", "seed_noisy_optimal_many"]
