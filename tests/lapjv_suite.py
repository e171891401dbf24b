"""Reader of the lapjv known-answer suite fixtures (tests/golden/lapjv_suite_*.npz).

The cases are those of the reference's LAP/lap/tests/test_lapjv.py plus NaN matrices of our own
recipe; tests/golden/make_golden.py (make_reference_suite) wrote the fixtures from the reference
build.  Matrices are stored as data (the small inf ones, eps) or rebuilt here from a stored recipe
(the integer ones by solvers.generators.known_answer_int_costs, checked against a stored sha256;
the NaN ones by solvers.generators.nan_costs).  Outputs: the reference's cold `(ret, x, y)` and
seeded `(ret, x, y)` for zero seeds and, where finite, row-min + min-trick seeds.

Cases of test_lapjv.py that are not square, unlimited `lapjv` calls -- and so not in this suite:
  * test_lapjv_extension (extend_cost=True), test_lapjv_cost_limit (cost_limit < inf) and
    test_arr_loop.py::test_lapjv_arr_loop (extend_cost=True on a 7x3 matrix): not supported,
    `lap.lapjv` raises NotImplementedError (tests/test_gpu_reference_suite.py asserts it);
  * test_square (KNOWN_SQUARE), test_lapjv_empty, test_lapjv_non_square_fail,
    test_lapjv_non_contigous, test_lapjv_noextension: tests/test_host_logic.py and
    tests/test_gpu_parity.py (test_reference_known_answers, test_solver_wrappers_and_error_behaviour).
"""
from __future__ import annotations

import hashlib
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"

INF5 = ("sparse_square", "infs_unsolvable_0", "infs_unsolvable_1", "inf_col", "inf_row", "all_inf")
INF4 = ("inf_unique",)
INF_LABELS = INF5 + INF4
UNSOLVABLE = ("infs_unsolvable_0", "infs_unsolvable_1", "inf_col", "inf_row", "all_inf")
EPS_OPT = 224.8899507294651


def sha256(C: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(C, dtype=np.float64).tobytes()).hexdigest()


class Suite:
    def __init__(self):
        self.z = np.load(GOLDEN / "lapjv_suite_cases.npz", allow_pickle=False)
        self.int_labels = [str(s) for s in self.z["int_labels"]]
        self.nan_labels = [str(s) for s in self.z["nan_labels"]]
        self.labels = list(INF_LABELS) + ["eps"] + self.int_labels + self.nan_labels
        self._mats = {}

    # ---- inputs
    def int_spec(self, label):
        k = self.int_labels.index(label)
        z = self.z
        return dict(n=int(z["int_n"][k]), hard=bool(z["int_hard"][k]), density=float(z["int_density"][k]),
                    fill=float(z["int_fill"][k]))

    def matrix(self, label) -> np.ndarray:
        """The cost matrix (a cached array: callers must not modify it)."""
        if label not in self._mats:
            from solvers.generators import known_answer_int_costs, nan_costs
            z = self.z
            if label in INF_LABELS:
                k = [str(s) for s in z["labels"]].index(label)
                n = int(z["n"][k])
                om = int(z["off_mat"][k])
                C = z["C"][om:om + n * n].reshape(n, n).copy()
            elif label == "eps":
                C = np.load(GOLDEN / "lapjv_suite_eps.npz", allow_pickle=False)["C"]
            elif label in self.int_labels:
                C = known_answer_int_costs(**self.int_spec(label))
            else:
                n, frac, col0, seed = self.z["nan_spec"][self.nan_labels.index(label)]
                C = nan_costs(int(n), float(frac), float(col0), int(seed))
            C.setflags(write=False)
            self._mats[label] = C
        return self._mats[label]

    def seed_kinds(self, label):
        return [s for s in ("zero", "rowmin") if f"{s}_ret__{label}" in self.z.files]

    def seeds(self, label, kind):
        C = self.matrix(label)
        n = C.shape[0]
        if kind == "zero":
            return np.zeros(n), np.zeros(n)
        u = C.min(1)
        with np.errstate(invalid="ignore"):
            v = (C - u[:, None]).min(0)
        return u, v

    # ---- the reference's outputs
    def cold(self, label):
        z = self.z
        return int(z[f"cold_ret__{label}"]), z[f"cold_x__{label}"], z[f"cold_y__{label}"]

    def seeded(self, label, kind):
        z = self.z
        return int(z[f"{kind}_ret__{label}"]), z[f"{kind}_x__{label}"], z[f"{kind}_y__{label}"]

    def opt(self, label):
        """test_lapjv.py's known optimum, or None (NaN cases, s4608)."""
        key = f"opt__{label}"
        if key not in self.z.files or np.isnan(self.z[key]):
            return None
        return float(self.z[key])

    def known_x(self, label):
        key = f"known_x__{label}"
        return self.z[key] if key in self.z.files else None


def assert_known_optimum(suite: Suite, label: str, opt: float):
    """The optimum test_lapjv.py asserts for `label` (nothing where it asserts none)."""
    want = suite.opt(label)
    if want is None:
        return
    if label == "eps":
        assert opt == pytest.approx(EPS_OPT, rel=1e-13), (label, opt)
    elif np.isinf(want):
        assert opt == np.inf, (label, opt)
    else:
        assert opt == want, (label, opt, want)
