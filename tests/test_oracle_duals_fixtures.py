"""CPU checks of the oracle-duals fixtures (tests/golden/oracle_duals_cases.npz, written by
tests/golden/make_oracle_duals.py from the reference) and of the two facts the device
implementation rests on: synchronous (Jacobi) sweeps reach the reference's v, and np.mean is
numpy's pairwise sum divided by n."""
import numpy as np
import pytest

from oracle_duals_common import OracleCases, jacobi, oracle_from_v, pairwise_sum, sha

CASES = OracleCases()
DIFF = CASES.indices("diff")


def test_public_surface_imports():
    from solvers import (check_dual_and_match, compute_oracle_duals,  # noqa: F401
                         dual_from_matching_diff_constraints, make_feasible_duals, verify_solver_correctness)


def test_fixture_inventory():
    labels = [m["label"] for m in CASES.meta]
    for fam in ("uniform", "sparse", "tie", "noisy_linear", "metric", "clustered"):
        for n in (16, 64, 256, 512):
            assert f"{fam}_n{n}" in labels
    for lab in ("uniform_n1024", "sparse_n1024", "n1", "n2", "nonopt_n8", "nonopt_uniform_n512",
                "int100_n64", "int100_n256", "search_assertion", "oracle_fallback_n1"):
        assert lab in labels, lab
    outcomes = {m["outcome"] for m in CASES.meta if m["kind"] == "diff"}
    assert outcomes == {"ok", "RuntimeError", "AssertionError"}
    deep_ok = [m for m in CASES.meta if m["kind"] == "diff" and m["outcome"] == "ok" and m["sweeps"] - 1 > m["n"] - 2]
    assert deep_ok, "no case where the Jacobi sweeps exceed n - 2 and the reference still succeeds"


@pytest.mark.parametrize("k", range(len(CASES)), ids=[m["label"] for m in CASES.meta])
def test_fixture_digest(k):
    m = CASES.case(k)
    assert sha(m["C"]) == m["sha_C"]


@pytest.mark.parametrize("k", DIFF, ids=[CASES.meta[k]["label"] for k in DIFF])
def test_jacobi_restatement_reproduces_reference(k):
    m = CASES.case(k)
    C, rows, cols, n = m["C"], m["rows"], m["cols"], m["n"]
    v, sweeps = jacobi(C, rows, cols)
    assert sweeps == m["sweeps"]
    if sweeps != -1 and sweeps - 1 <= n - 2:
        # the reference's loop breaks: no negative-cycle error
        assert m["outcome"] != "RuntimeError"
    if m["outcome"] == "ok":
        u, v = oracle_from_v(C, rows, cols, v)
        assert np.array_equal(u.view(np.int64), m["u"].view(np.int64))
        assert np.array_equal(v.view(np.int64), m["v"].view(np.int64))
        red = C - u[:, None] - v[None, :]
        assert sha(red) == m["sha_red"]


@pytest.mark.parametrize("n", [1, 2, 5, 7, 8, 9, 15, 16, 17, 100, 127, 128, 129, 130, 255, 256, 257, 1000,
                               2047, 2048, 2049, 4099, 8191, 8192, 8193, 12345, 16383, 16384])
def test_pairwise_mean_restatement(n):
    a = np.random.default_rng(n).standard_normal(n) * 1e3
    assert pairwise_sum(a.tolist()) / n == np.mean(a)
