"""Sparse LAPMOD without a GPU: argument errors and their texts, which precede device work; the CSR helpers and
get_cost against the stored fixtures; the ABI surface; `lap.lapmod` itself still raising."""
import ctypes as ct
import re

import numpy as np
import pytest

from conftest import ROOT
from host_common import lib  # noqa: F401
from lapmod_common import densify, load_cases, long_row_labels, problem

ENTRIES = {"lapwarm_lapmod_workspace_bytes": 3, "lapwarm_lapmod_lds_max_n": 0, "lapwarm_lapmod_ragged": 18}


def test_entries_are_declared_bound_and_exported(lib):
    from lap import _hip
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in lapwarm_hip.h"
        assert hasattr(lib, name), name
        assert len(_hip.SIGNATURES[name][1]) == n_args, name
        if n_args:
            assert m.group(1).count(",") + 1 == n_args, name


def test_lds_bound_follows_from_the_layout(lib):
    bound = lib.lapwarm_lapmod_lds_max_n()

    def state_bytes(n):  # v, d fp64; x, y, pred, free_rows, three lists, rev_kk int32; two bitmaps
        return (16 * n + 32 * n + 8 * ((n + 31) // 32) + 15) & ~15

    assert state_bytes(bound) <= 160 * 1024 < state_bytes(bound + 1)
    assert bound == load_cases()[1]


def test_workspace_query(lib):
    bound = lib.lapwarm_lapmod_lds_max_n()

    def query(sizes, nnz=None):
        arr = (ct.c_int * len(sizes))(*sizes)
        nz = (ct.c_longlong * len(sizes))(*nnz) if nnz is not None else None
        return lib.lapwarm_lapmod_workspace_bytes(arr, nz, len(sizes))

    small = query([5, bound, 128])
    assert 0 < small <= 4096  # offsets only: every state is in LDS
    big = query([5, bound + 1, 128, 16384])
    assert big - small >= 48 * (bound + 1) + 48 * 16384
    assert big - small <= 49 * (bound + 1 + 16384) + 1024
    assert query([0]) == 0 and query([-3, 4]) == 0 and query([65536]) == 0 and query([65535]) > 0
    assert query([4], [17]) == 0 and query([4], [16]) > 0
    assert lib.lapwarm_lapmod_workspace_bytes(None, None, 1) == 0
    assert lib.lapwarm_lapmod_workspace_bytes((ct.c_int * 1)(4), None, 0) == 0


def test_argument_errors_return_before_any_launch(lib):
    sizes = (ct.c_int * 2)(4, 6)
    p = ct.c_void_p(4096)  # never dereferenced: every call below returns before device work

    def call(batch=2, N=6, fp=3, host=sizes, cc=p, x=p, ws=p, nbytes=1 << 20):
        return lib.lapwarm_lapmod_ragged(cc, p, p, p, p, p, host, batch, N, fp, x, p, None, p, None, ws, nbytes, None)

    assert call(batch=0) == -2 and call(batch=65536) == -2
    assert call(N=0) == -2 and call(N=5) == -2  # a host size above N
    assert call(fp=0) == -2 and call(fp=4) == -2
    assert call(host=None) == -2 and call(cc=None) == -2 and call(x=None) == -2 and call(ws=None) == -2
    assert call(ws=ct.c_void_p(4104)) == -2  # not 16-byte aligned
    assert call(N=65536) == -5
    assert call(nbytes=8) == -1


def test_python_argument_errors_precede_device_work():
    import lap
    from lap import lapmod_sparse, lapmod_many  # noqa: F401  (ImportError where the sparse solver is missing)
    cases, _ = load_cases()
    n, cc, ii, kk = problem(cases["known8_masked"])
    with pytest.raises(ValueError, match="at most 65535"):
        lap.lapmod_sparse(65536, cc, ii, kk)
    empty_f, empty_i = np.zeros(0), np.zeros(0, dtype=int)
    with pytest.raises(ValueError, match="Cost matrix has zero rows."):
        lap.lapmod_sparse(0, empty_f, np.zeros(1, dtype=int), empty_i)
    with pytest.raises(ValueError, match="Cost matrix has zero columns."):
        lap.lapmod_sparse(2, empty_f, np.zeros(3, dtype=int), empty_i)
    bad = cc.copy()
    bad[3] = -1.0
    with pytest.raises(ValueError, match="Cost matrix values must be non-negative."):
        lap.lapmod_sparse(n, bad, ii, kk)
    bad[3] = 1e6
    with pytest.raises(ValueError, match="Cost matrix values must be less than 1000000"):
        lap.lapmod_sparse(n, bad, ii, kk)
    bad[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        lap.lapmod_sparse(n, bad, ii, kk)
    for fp in (0, 4, 99, True):
        with pytest.raises(ValueError, match="fp_version"):
            lap.lapmod_sparse(n, cc, ii, kk, fp_version=fp)
    swapped = kk.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(ValueError, match="sorted"):
        lap.lapmod_sparse(n, cc, ii, swapped)
    wide = kk.copy()
    wide[-1] = n
    with pytest.raises(ValueError, match="0..n-1"):
        lap.lapmod_sparse(n, cc, ii, wide)
    for bad_ii in (ii[:-1], ii + 1, np.r_[ii[:-1], ii[-1] - 1], np.r_[0, ii[2], ii[1], ii[3:]]):
        with pytest.raises(ValueError, match="ii must hold"):
            lap.lapmod_sparse(n, cc, bad_ii, kk)
    with pytest.raises(ValueError, match="sorted"):
        lap.lapmod_many([(n, cc, ii, kk), (n, cc, ii, swapped)])
    with pytest.raises(ValueError, match=r"\(n, cc, ii, kk\)"):
        lap.lapmod_many([(n, cc, ii)])
    with pytest.raises(TypeError):
        lap.lapmod_many(None)
    assert lap.lapmod_many([]) == []
    from solvers import LAPMODSolver
    with pytest.raises(ValueError, match="fp_version"):
        LAPMODSolver().solve(np.ones((3, 3)), fp_version=7)


def test_lapmod_still_raises_and_new_names_are_unlisted():
    import lap
    import solvers
    from lap._lapmod import lapmod_sparse  # noqa: F401  (ImportError where the sparse solver is missing)
    with pytest.raises(NotImplementedError):
        lap.lapmod()
    for name in ("lapmod_sparse", "lapmod_many", "get_cost", "sparse_from_dense", "sparse_from_masked"):
        assert callable(getattr(lap, name)) and name not in lap.__all__
    assert "lapmod_sparse" in lap.__doc__ and "__all__" in lap.__doc__
    assert solvers.LAPMODSolver().name == "LAPMOD" and "LAPMODSolver" in solvers.__all__


def test_sparse_helpers_match_the_fixtures():
    import lap
    from lap import sparse_from_dense, sparse_from_masked  # noqa: F401  (ImportError on a tree without them)
    cases, _ = load_cases()
    for label in ("known8_dense", "known_square3", "n3_dense_cont"):
        c = cases[label]
        n, cc, ii, kk = lap.sparse_from_dense(densify(c))
        assert n == c["n"] and np.array_equal(cc, c["cc"]) and np.array_equal(ii, c["ii"])
        assert np.array_equal(kk, c["kk"])
    for label in ("known8_masked", "inf_row", "inf_unique", "n65_sparse_tie", "empty_column"):
        c = cases[label]
        D = densify(c)
        for args in ((D,), (np.where(np.isinf(D), -5.0, D), np.isfinite(D))):
            n, cc, ii, kk = lap.sparse_from_masked(*args)
            assert n == c["n"] and np.array_equal(cc, c["cc"]) and np.array_equal(ii, c["ii"])
            assert np.array_equal(kk, c["kk"])


def test_long_row_cases_keep_what_they_are_there_for():
    """What tests/golden/make_lapmod.py asserts of lapmod_long_rows.npz when it writes it, read back from the file:
    a regeneration cannot lose the long rows, the inexact costs in the search or the rows that start above LARGE."""
    cases, _ = load_cases()
    labels = long_row_labels()
    assert labels == ("dec_full129", "dec_full193", "dec_rows64_n130", "dec_rows65_n130", "dec_rows128_n200",
                      "dec_rows129_n200", "dec_sparse130", "lowrank129", "dec_single193", "dec_empty_col130",
                      "dec_hall130")
    assert list(cases)[-len(labels):] == list(labels) and len(cases) == 45 + len(labels)
    lengths, picked = set(), set()
    for label in labels:
        c = cases[label]
        lengths |= set(np.diff(c["ii"]).tolist())
        assert not np.all(c["cc"] * 64 == np.floor(c["cc"] * 64)), label  # no dyadic costs: fp64 rounds
        assert np.all(c["cc"] >= 0.0) and np.all(c["cc"] < 1e6), label
        assert c["solvable"] == (label not in ("dec_empty_col130", "dec_hall130")), label
        if c["solvable"]:
            assert c["aug"], label  # the path search runs
            assert set(c["ref"]) == {1, 2, 3} and set(c["v"]) == {1, 2, 3}, label
            picked.add(c["dyn"])
        else:
            assert c["strict"] and c["n"] > 64 and c["dyn"] == 1 and set(c["ref"]) == {1, 3}, label
    assert {64, 65, 128, 129, 193} <= lengths
    assert picked == {1, 2}
    assert cases["dec_sparse130"]["dyn"] == 2 and cases["dec_full129"]["dyn"] == 1
    tenths = cases["dec_full193"]["cc"]
    assert np.array_equal(tenths, np.rint(tenths * 10) / 10.0) and set(np.rint(tenths * 10)) == set(range(1, 8))
    single = cases["dec_single193"]
    assert single["arr_first_above"] >= 1 and single["arr_first_far"] >= 1
    assert single["arr_first_far"] <= single["arr_first_above"]
    assert 1 in np.diff(single["ii"]) and 193 in np.diff(single["ii"])
    hall = cases["dec_hall130"]
    assert np.unique(hall["kk"]).size == hall["n"] and np.sum(np.diff(hall["ii"]) == 1) == 2
    empty = cases["dec_empty_col130"]
    assert np.unique(empty["kk"]).size == empty["n"] - 1 and np.all(np.diff(empty["ii"]) > 0)
    # the 45 earlier cases reach none of this: rows of at most 103 entries
    assert max(np.diff(c["ii"]).max() for label, c in cases.items() if label not in labels) == 103


def test_get_cost_matches_the_fixtures():
    import lap
    from lap import get_cost  # noqa: F401  (ImportError on a tree without it)
    cases, _ = load_cases()
    known = {"known8_dense": 17.0, "known8_masked": 17.0, "known_square0": 3.0, "known_square7": 41.0,
             "known_sparse_square": 71.0, "inf_unique": 3.0}
    for label, c in cases.items():
        if not c["solvable"] or c["n"] > 300:
            continue
        D = densify(c)
        for fp, (ret, x, y) in c["ref"].items():
            got = lap.get_cost(*problem(c), x)
            want = 0
            for i in range(c["n"]):  # left to right, as the reference sums
                want += D[i, x[i]]
            assert ret == 0 and got == want and np.isfinite(got), (label, fp)
            if label in known:
                assert got == known[label], label
    c = cases["known8_masked"]
    assert lap.get_cost(*problem(c), np.arange(8)) == np.inf  # the masked diagonal
    assert lap.get_cost(*problem(c), np.full(8, -1)) == np.inf
