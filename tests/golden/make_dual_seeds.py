#!/usr/bin/env python3
"""Generate tests/golden/dual_seeds_cases.npz FROM THE REFERENCE.

Runs only where the reference repository exists (oracle/ref.py knows where).  It loads the reference's
solvers/advanced_dual.py and solvers/seed_baselines.py through oracle.ref.load_module (imported, never copied) and
stores
inputs and outcomes as data:

  * cost matrices at n in SIZES: `uni` (uniform) and `int` (integers 0..4, many ties) directly; `inf` and
    `nan` as a patch of `uni` (flat indices and the values written there: +inf, one -inf, or one NaN);
  * seeds per matrix: `rc` (row/col minima before projection), `noisy` (rc plus N(0, 0.05) from
    default_rng), `infeas` (uniform in [0, 1): infeasible), `low` (all -10: no column is ever capped);
  * project_feasible for every (max_rounds, tol) of ROUNDS x TOLS: the reference's u, v are stored once per
    number of rounds the call ran (`u__<case>__r<k>`), `rounds__<case>` is the [len(ROUNDS)][len(TOLS)] table
    of those numbers and `gmin__<case>__r<k>` the min reduced cost of the stored u, v;
  * reduce_costs with shift_nonneg on and off for a subset (reduced_in_subset), check_dual_feasible outcomes for all;
  * seed_row_col_minima for every matrix; seed_noisy_optimal for uniform matrices `C__opt_n<n>` (continuous costs,
    unique optimum), drawn from ONE default_rng(NOISY_SEED) over NOISY_SIZES in order.

Usage:  python tests/golden/make_dual_seeds.py          (from the repo root)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from oracle.ref import load_module  # noqa: E402

OUT = Path(__file__).resolve().parent / "dual_seeds_cases.npz"

SIZES = (1, 2, 7, 33, 64, 65)
KINDS = ("uni", "int", "inf", "nan")
SEEDS = ("rc", "noisy", "infeas", "low")
ROUNDS = (0, 1, 3)
TOLS = (1e-12, -1e-3, -0.5)
NOISY_SEED = 7
NOISY_SIZES = (2, 7, 33, 64, 65)


# seed_baselines imports `.advanced_dual` and `.dual_computation`: all three live in one stand-in package
load_module("solvers/dual_computation.py", "dual_computation", package="_ref_solvers")
ref_ad = load_module("solvers/advanced_dual.py", "advanced_dual", package="_ref_solvers")
ref_sb = load_module("solvers/seed_baselines.py", "seed_baselines", package="_ref_solvers")


def reduced_in_subset(n, kind, seed):
    return seed == "infeas" and (n <= 33 or kind == "uni")


def rounds_run(C, u, v, max_rounds, tol):
    """How many rounds project_feasible runs: a count only, the stored u, v come from the reference."""
    u, v = u.copy(), v.copy()
    k = 0
    for _ in range(max(1, int(max_rounds))):
        k += 1
        u = np.minimum(u, (C - v[None, :]).min(axis=1))
        v = np.minimum(v, (C - u[:, None]).min(axis=0))
        if (C - u[:, None] - v[None, :]).min() >= -tol:
            break
    return k


def main():
    out = {"sizes": np.array(SIZES), "kinds": np.array(KINDS), "seeds": np.array(SEEDS),
           "max_rounds": np.array(ROUNDS), "tols": np.array(TOLS), "noisy_seed": np.array(NOISY_SEED),
           "noisy_sizes": np.array(NOISY_SIZES)}
    reduced_cases = []
    with np.errstate(invalid="ignore"):
        for n in SIZES:
            rng = np.random.default_rng(1000 + n)
            uni = rng.random((n, n))
            mats = {"uni": uni, "int": rng.integers(0, 5, size=(n, n)).astype(np.float64)}
            out[f"C__uni_n{n}"] = uni
            out[f"C__int_n{n}"] = mats["int"].astype(np.int8)
            k = max(1, n // 4)
            idx = rng.choice(n * n, size=min(n * n, k + 1), replace=False)
            val = np.full(idx.shape, np.inf)
            if n >= 2:
                val[-1] = -np.inf
            out[f"patch_idx__inf_n{n}"], out[f"patch_val__inf_n{n}"] = idx, val
            out[f"patch_idx__nan_n{n}"] = rng.choice(n * n, size=1)
            out[f"patch_val__nan_n{n}"] = np.array([np.nan])
            for kind in ("inf", "nan"):
                C = uni.copy()
                C.reshape(-1)[out[f"patch_idx__{kind}_n{n}"]] = out[f"patch_val__{kind}_n{n}"]
                mats[kind] = C
            for kind in KINDS:
                C = mats[kind]
                mk = f"{kind}_n{n}"
                su, sv = ref_sb.seed_row_col_minima(C)
                out[f"rcseed_u__{mk}"], out[f"rcseed_v__{mk}"] = su, sv
                u_rc = C.min(axis=1)
                v_rc = (C - u_rc[:, None]).min(axis=0)
                srng = np.random.default_rng(2000 + n)
                seeds = {"rc": (u_rc, v_rc),
                         "noisy": (u_rc + srng.normal(0.0, 0.05, n), v_rc + srng.normal(0.0, 0.05, n)),
                         "infeas": (srng.random(n), srng.random(n)),
                         "low": (np.full(n, -10.0), np.full(n, -10.0))}
                for seed, (u0, v0) in seeds.items():
                    case = f"{mk}_{seed}"
                    out[f"u0__{case}"], out[f"v0__{case}"] = u0, v0
                    table = np.zeros((len(ROUNDS), len(TOLS)), dtype=np.int32)
                    for a, mr in enumerate(ROUNDS):
                        for b, tol in enumerate(TOLS):
                            pu, pv = ref_ad.project_feasible(C, u0, v0, max_rounds=mr, tol=tol)
                            r = rounds_run(C, u0, v0, mr, tol)
                            table[a, b] = r
                            key = f"{case}__r{r}"
                            if f"u__{key}" in out:
                                assert np.array_equal(out[f"u__{key}"], pu, equal_nan=True), key
                                assert np.array_equal(out[f"v__{key}"], pv, equal_nan=True), key
                            else:
                                out[f"u__{key}"], out[f"v__{key}"] = pu, pv
                                out[f"gmin__{key}"] = np.array((C - pu[:, None] - pv[None, :]).min())
                    out[f"rounds__{case}"] = table
                    try:
                        ref_ad.check_dual_feasible(C, u0, v0)
                        feas = True
                    except AssertionError:
                        feas = False
                    out[f"feasible__{case}"] = np.array(feas)
                    if reduced_in_subset(n, kind, seed):
                        reduced_cases.append(case)
                        out[f"red_shift__{case}"] = ref_ad.reduce_costs(C, u0, v0, True)
                        if n <= 33:
                            out[f"red_noshift__{case}"] = ref_ad.reduce_costs(C, u0, v0, False)
        # The reference's difference-constraint step raises "Negative cycle" for every 1 x 1 matrix and for most
        # 2 x 2 ones (before it draws anything): n = 1 is left out and the first matrix it accepts is taken.
        rng = np.random.default_rng(NOISY_SEED)
        for n in NOISY_SIZES:
            for s in range(8):
                C = np.random.default_rng(3000 + 10 * n + s).random((n, n))
                try:
                    u, v = ref_sb.seed_noisy_optimal(C, noise_std=0.05, rng=rng)
                except RuntimeError:
                    continue
                break
            else:
                raise SystemExit(f"no matrix of size {n} that the reference accepts")
            out[f"C__opt_n{n}"], out[f"noisyopt_u__n{n}"], out[f"noisyopt_v__n{n}"] = C, u, v
    out["reduced_cases"] = np.array(reduced_cases)
    np.savez_compressed(OUT, **out)
    print(f"{OUT.name}: {len(out)} arrays, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
