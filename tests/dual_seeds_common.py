"""Shared by the dual-seed tests: the fixture tests/golden/dual_seeds_cases.npz (written by
tests/golden/make_dual_seeds.py from the reference) and plain NumPy statements of the formulas it pins."""
import functools
import warnings

import numpy as np

from conftest import GOLDEN

FIXTURE = GOLDEN / "dual_seeds_cases.npz"


def quiet_warnings(fn):
    """inf - inf and NaN comparisons are part of the cases: no RuntimeWarning for them."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            return fn(*args, **kwargs)
    return wrapped


def same(a, b):
    """Equal numbers, NaN exactly where the other has NaN (what np.array_equal is without NaN)."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@functools.lru_cache(maxsize=None)
def cases():
    return np.load(FIXTURE, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    z = cases()
    if kind in ("uni", "int", "opt"):
        C = z[f"C__{kind}_n{n}"].astype(np.float64)
    else:
        C = z[f"C__uni_n{n}"].copy()
        C.reshape(-1)[z[f"patch_idx__{kind}_n{n}"]] = z[f"patch_val__{kind}_n{n}"]
    C.setflags(write=False)
    return C


def case_names():
    z = cases()
    return [(str(k), int(n), str(s)) for n in z["sizes"] for k in z["kinds"] for s in z["seeds"]]


def case_key(kind, n, seed):
    return f"{kind}_n{n}_{seed}"


def combos():
    z = cases()
    return [(a, b, int(mr), float(tol)) for a, mr in enumerate(z["max_rounds"]) for b, tol in enumerate(z["tols"])]


@quiet_warnings
def np_project(C, u, v, max_rounds=50, tol=1e-12, two_read=False):
    """project_feasible as the formulas read: (u, v, gmin of the last round, rounds run).  two_read: gmin from
    the column pass, min_j (cap_j - v_j), instead of a third sweep over C."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    rounds, gmin = 0, None
    for _ in range(max(1, int(max_rounds))):
        rounds += 1
        u = np.minimum(u, (C - v[None, :]).min(axis=1))
        cap = (C - u[:, None]).min(axis=0)
        v = np.minimum(v, cap)
        gmin = (cap - v).min() if two_read else ((C - u[:, None]) - v[None, :]).min()
        if gmin >= -tol:
            break
    return u, v, gmin, rounds


@quiet_warnings
def np_reduce(C, u, v, shift_nonneg=True):
    """reduce_costs: (matrix, unshifted minimum)."""
    red = (C - u[:, None]) - v[None, :]
    m = red.min()
    if shift_nonneg and m < 0:
        red = red - m
    return red, m


@quiet_warnings
def np_seed_row_col_minima(C, project_rounds=50):
    u = C.min(axis=1)
    v = (C - u[:, None]).min(axis=0)
    return np_project(C, u, v, project_rounds)[:2]
