#!/usr/bin/env python3
"""Generate tests/golden/oracle_duals_cases.npz FROM THE REFERENCE.

Runs only where the reference repository exists (oracle/ref.py knows where).  It loads the reference's
solvers/dual_computation.py and solvers/advanced_dual.py through oracle.ref.load_module (imported, never
copied), takes the matching from SciPy's linear_sum_assignment as the reference does, and
stores inputs and outcomes as data:

  * matrices as a `generate_family` recipe (family, n, seed) plus the sha256 of C; small or
    hand-made matrices directly;
  * per case: rows, cols, the outcome (ok / RuntimeError / AssertionError and its message),
    u, v, the sha256 of `red`, and the number of Jacobi sweeps (the last one changes nothing);
  * compute_oracle_duals and make_feasible_duals outputs for a few instances.

Usage:  python tests/golden/make_oracle_duals.py          (from the repo root)
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.optimize

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "oracle_duals_cases.npz"
sys.path[:0] = [str(ROOT), str(ROOT / "gnn-accelerated-lap-warm-start-pipeline_amd")]

from oracle.ref import load_module  # noqa: E402
from solvers import generators as gen  # noqa: E402

# advanced_dual.make_feasible_duals imports `.dual_computation`: both live in one stand-in package
ref_dc = load_module("solvers/dual_computation.py", "dual_computation", package="_ref_solvers")
ref_ad = load_module("solvers/advanced_dual.py", "advanced_dual", package="_ref_solvers")


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def jacobi_sweeps(C, rows, cols, cap):
    """Synchronous sweeps from v = 0 until one changes nothing (at most `cap` sweeps)."""
    n = C.shape[1]
    W = C[rows, :] - C[rows, cols][:, None]
    v = np.zeros(n)
    for s in range(1, cap + 1):
        cand = (v[cols][:, None] + W).min(axis=0)
        nv = np.where(v > cand, cand, v)
        if np.array_equal(nv, v):
            return s
        v = nv
    return -1


def int_family(name, n, seed):
    rs = np.random.RandomState(seed)
    if name == "int100":
        return rs.randint(1, 101, size=(n, n)).astype(np.float64)
    raise KeyError(name)


def make_C(recipe):
    fam, n, seed = recipe
    return int_family(fam, n, seed) if fam.startswith("int") else gen.generate_family(fam, n, seed)


cases = []      # meta dicts
arrays = {}     # npz payload


def add_diff_case(label, C, rows, cols, recipe=None):
    k = len(cases)
    t = time.time()
    meta = dict(label=label, kind="diff", n=int(C.shape[0]), sha_C=sha(C))
    if recipe is not None:
        meta["recipe"] = list(recipe)
    else:
        arrays[f"c{k}_C"] = C
    rows = np.asarray(rows, dtype=np.int32)
    cols = np.asarray(cols, dtype=np.int32)
    arrays[f"c{k}_rows"] = rows
    arrays[f"c{k}_cols"] = cols
    try:
        u, v, red = ref_dc.dual_from_matching_diff_constraints(C, rows.astype(np.int64), cols.astype(np.int64))
        meta.update(outcome="ok", message="", sha_red=sha(red))
        arrays[f"c{k}_u"] = u
        arrays[f"c{k}_v"] = v
    except (RuntimeError, AssertionError) as e:
        meta.update(outcome=type(e).__name__, message=str(e))
    n = C.shape[0]
    meta["sweeps"] = jacobi_sweeps(C, rows, cols, cap=n + 2)
    cases.append(meta)
    print(f"{label:40s} {meta['outcome']:15s} sweeps {meta['sweeps']:4d}  {time.time() - t:6.1f} s", flush=True)


def add_family_case(fam, n, seed=7):
    C = make_C((fam, n, seed))
    r, c = scipy.optimize.linear_sum_assignment(C)
    add_diff_case(f"{fam}_n{n}", C, r, c, recipe=(fam, n, seed))


# ---- 1. families on SciPy's optimal matching
# (not low_rank: its rank-12 matrix product rounds differently with different BLAS builds, so a
# recipe would not rebuild the same matrix everywhere)
for n in (16, 64, 256, 512):
    for fam in ("uniform", "sparse", "tie", "noisy_linear", "metric", "clustered"):
        add_family_case(fam, n)
for fam in ("uniform", "sparse"):
    add_family_case(fam, 1024)
for n in (64, 256):
    add_family_case("int100", n)

# ---- 2. n = 1 and n = 2
add_diff_case("n1", np.array([[3.5]]), [0], [0])
add_diff_case("n2", np.array([[1.0, 2.0], [3.0, 1.5]]), [0, 1], [0, 1])
add_diff_case("n2_swapped_pairs", np.array([[4.0, 1.0], [2.0, 7.0]]), [1, 0], [0, 1])

# ---- 3. searched small matrices: J > n - 2 with success; a raise on an optimal matching
rs = np.random.RandomState(2024)
found_deep_ok = found_raise = 0
for trial in range(4000):
    if found_deep_ok >= 2 and found_raise >= 2:
        break
    n = int(rs.randint(3, 7))
    C = rs.randint(0, 20, size=(n, n)).astype(np.float64) if trial % 2 else rs.uniform(0, 10, size=(n, n))
    r, c = scipy.optimize.linear_sum_assignment(C)
    s = jacobi_sweeps(C, r, c, cap=n + 2)
    if s - 1 <= n - 2:
        continue
    try:
        ref_dc.dual_from_matching_diff_constraints(C, r, c)
        if found_deep_ok < 2:
            found_deep_ok += 1
            add_diff_case(f"search_deep_ok_{found_deep_ok}", C, r, c)
    except (RuntimeError, AssertionError):
        if found_raise < 2:
            found_raise += 1
            add_diff_case(f"search_raise_{found_raise}", C, r, c)

# large magnitudes: rounding at 1e12 exceeds the 1e-6 slackness tolerance
for seed in range(50):
    C = np.random.RandomState(seed).uniform(1e12, 2e12, size=(8, 8))
    r, c = scipy.optimize.linear_sum_assignment(C)
    try:
        ref_dc.dual_from_matching_diff_constraints(C, r, c)
    except AssertionError:
        add_diff_case("search_assertion", C, r, c)
        break
    except RuntimeError:
        continue
else:
    print("no AssertionError case found", flush=True)

# ---- 4. non-optimal matchings (a rotation of the optimum)
C8 = np.random.RandomState(5).uniform(0, 1, size=(8, 8))
r, c = scipy.optimize.linear_sum_assignment(C8)
add_diff_case("nonopt_n8", C8, r, np.roll(c, 1))
C512 = make_C(("uniform", 512, 11))
r, c = scipy.optimize.linear_sum_assignment(C512)
add_diff_case("nonopt_uniform_n512", C512, r, np.roll(c, 1), recipe=("uniform", 512, 11))

# ---- 5. compute_oracle_duals (noise 0 / 0.1, a fallback) and make_feasible_duals
def add_oracle_case(label, C, noise, recipe=None):
    k = len(cases)
    meta = dict(label=label, kind="oracle", n=int(C.shape[0]), sha_C=sha(C), noise=noise)
    if recipe is not None:
        meta["recipe"] = list(recipe)
    else:
        arrays[f"c{k}_C"] = C
    r, c = scipy.optimize.linear_sum_assignment(C)
    arrays[f"c{k}_cols"] = c.astype(np.int32)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        u, v = ref_dc.compute_oracle_duals(C, noise_level=noise)
    meta["fallback"] = "Warning: Difference constraints failed" in buf.getvalue()
    meta["printed"] = buf.getvalue()
    arrays[f"c{k}_u"] = u
    arrays[f"c{k}_v"] = v
    cases.append(meta)
    print(f"{label:40s} oracle fallback={meta['fallback']}", flush=True)


def add_feasible_case(label, C, noise_std, recipe):
    k = len(cases)
    meta = dict(label=label, kind="feasible", n=int(C.shape[0]), sha_C=sha(C), noise_std=noise_std,
                recipe=list(recipe))
    r, c = scipy.optimize.linear_sum_assignment(C)
    arrays[f"c{k}_cols"] = c.astype(np.int32)
    u, v = ref_ad.make_feasible_duals(C, noise_std=noise_std)
    arrays[f"c{k}_u"] = u
    arrays[f"c{k}_v"] = v
    cases.append(meta)
    print(f"{label:40s} feasible", flush=True)


for fam, n in (("uniform", 64), ("noisy_linear", 256)):
    C = make_C((fam, n, 3))
    for noise in (0.0, 0.1):
        add_oracle_case(f"oracle_{fam}_n{n}_noise{noise}", C, noise, recipe=(fam, n, 3))
add_oracle_case("oracle_fallback_n1", np.array([[2.25]]), 0.0)
add_oracle_case("oracle_fallback_n1_noise", np.array([[2.25]]), 0.1)
for fam, n in (("uniform", 64), ("sparse", 256)):
    C = make_C((fam, n, 4))
    for ns in (0.0, 0.05):
        add_feasible_case(f"feasible_{fam}_n{n}_noise{ns}", C, ns, recipe=(fam, n, 4))

arrays["meta"] = np.array(json.dumps(cases))
np.savez_compressed(OUT, **arrays)
print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(cases)} cases)")
