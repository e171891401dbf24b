"""The pruned exact solve without a GPU: the ABI surface, argument errors (which precede device work), the NumPy
restatement against the stored fixture (where the reference builds exist) and the invariants of one grow step."""
import ctypes as ct
import re

import numpy as np
import pytest

from conftest import ROOT
from host_common import lib  # noqa: F401
from prune_common import (CASES, FAMILIES, admissible, family_matrix, grow, load_fixture, reference_lapmod,
                          solve_pruned, to_csr)

ENTRIES = {"lapwarm_prune_workspace_bytes": 2, "lapwarm_prune_grow_ragged": 25, "lapwarm_prune_finish_ragged": 12}


def test_entries_are_declared_bound_and_exported(lib):
    from lap import _hip
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in lapwarm_hip.h"
        assert hasattr(lib, name), name
        assert len(_hip.SIGNATURES[name][1]) == n_args, name
        assert m.group(1).count(",") + 1 == n_args, name


def test_workspace_query(lib):
    q = lib.lapwarm_prune_workspace_bytes
    assert q(0, 8) == 0 and q(65536, 8) == 0 and q(1, 0) == 0 and q(1, 16385) == 0
    assert 24 * 32 * 2048 <= q(32, 2048) <= 24 * 32 * 2048 + 5 * 256  # 8 + 4 * 4 bytes per row, five arrays
    assert q(1, 16384) > 0


def test_argument_errors_return_before_any_launch(lib):
    p = ct.c_void_p(4096)  # never dereferenced: every call below returns before device work
    csr_in, csr_out = [p] * 4, [p] * 6

    def call(C=p, ld=0, batch=2, N=6, key=p, x=p, cur=csr_in, m=4, out=csr_out, added=p, ws=p, nbytes=1 << 20):
        return lib.lapwarm_prune_grow_ragged(C, p, p, ld, batch, N, key, x, *cur, m, *out, added, p, p, ws, nbytes,
                                             None)

    assert call(batch=0) == -2 and call(batch=65536) == -2 and call(N=0) == -2 and call(ld=-1) == -2
    assert call(N=16385) == -5
    assert call(C=None) == -2 and call(added=None) == -2 and call(ws=None) == -2
    assert call(m=0) == -2 and call(m=257) == -2
    assert call(key=None) == -2  # x without a key vector
    assert call(cur=[p, p, None, p]) == -2 and call(cur=[None, p, p, p]) == -2  # a CSR given in part
    assert call(out=[p, p, p, p, p, None]) == -2 and call(out=[None, p, p, p, p, p]) == -2
    assert call(nbytes=8) == -1

    def finish(C=p, batch=2, N=6, x=p, cost=p):
        return lib.lapwarm_prune_finish_ragged(C, p, p, 0, batch, N, x, p, p, p, cost, None)

    assert finish(batch=0) == -2 and finish(N=0) == -2 and finish(C=None) == -2 and finish(x=None) == -2
    assert finish(cost=None) == -2 and finish(N=16385) == -5


def test_python_argument_errors_precede_device_work():
    import lap
    from lap import lapjv_pruned, lapjv_pruned_many  # noqa: F401  (ImportError on a tree without them)
    C = np.arange(16, dtype=np.float64).reshape(4, 4)
    with pytest.raises(ValueError, match="Square"):
        lap.lapjv_pruned(C[:3])
    with pytest.raises(ValueError, match="Square"):
        lap.lapjv_pruned(np.zeros((0, 0)))
    for k in (0, 257, -1):
        with pytest.raises(ValueError, match="k must be in 1..256"):
            lap.lapjv_pruned(C, k=k)
    for k in (True, 2.0, "4"):
        with pytest.raises(TypeError, match="'k'"):
            lap.lapjv_pruned(C, k=k)
    with pytest.raises(ValueError, match="length n"):
        lap.lapjv_pruned(C, v=np.zeros(3))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            lap.lapjv_pruned(C, v=np.array([0.0, bad, 0.0, 0.0]))
    with pytest.raises(ValueError, match="Square"):
        lap.lapjv_pruned_many([C, C[:2]])
    with pytest.raises(ValueError, match="one seed per cost matrix"):
        lap.lapjv_pruned_many([C, C], v=[np.zeros(4)])
    with pytest.raises(TypeError):
        lap.lapjv_pruned_many(None)
    assert lap.lapjv_pruned_many([]) == []
    for name in ("lapjv_pruned", "lapjv_pruned_many"):
        assert callable(getattr(lap, name)) and name not in lap.__all__
    assert "lapjv_pruned" in lap.__doc__


def test_case_list_covers_the_families_and_sizes():
    assert {c[1] for c in CASES} == set(FAMILIES)
    sizes = {c[2] for c in CASES}
    assert {1, 2, 63, 64, 65, 257, 600} <= sizes and len(sizes) >= 8 and max(sizes) <= 600
    assert {1, 4, 16, 64, 256} <= {c[3] for c in CASES}
    assert set(load_fixture()) == {c[0] for c in CASES}
    for label, family, n, k, seed in CASES:
        f = load_fixture()[label]
        assert (f["family"], f["n"], f["k"], f["seed"]) == (family, n, k, seed), label
        assert f["trace"][-1][1] == 0 and all(viol > 0 for _, viol in f["trace"][:-1]), label  # certified, once
        assert len(f["trace"]) <= 32, label
        assert admissible(family_matrix(family, n, seed)), label
    assert max(len(f["trace"]) for f in load_fixture().values()) >= 7  # some case needs many rounds


def test_restatement_reproduces_the_fixture():
    lapmod = reference_lapmod()
    if lapmod is None:
        pytest.skip("oracle/_ref is not built (the reference is not on this machine)")
    for label, family, n, k, seed in CASES:
        f = load_fixture()[label]
        C = family_matrix(family, n, seed)
        res = solve_pruned(C, k, lapmod, max_rounds=32)
        assert res["ret"] == 0 and res["trace"] == f["trace"], label
        assert np.array_equal(res["x"], f["x"]) and np.array_equal(res["v"].view(np.int64), f["v"].view(np.int64))
        assert res["cost"] == f["cost"], label


@pytest.mark.parametrize("family", FAMILIES)
def test_grow_gives_sorted_unique_rows_and_drops_nothing(family):
    n, m = 41, 5
    C = family_matrix(family, n, 99)
    rng = np.random.default_rng(7)
    rows, viol0 = grow(C, [np.array([i]) for i in range(n)], None, None, m)
    assert viol0 == n * (n - 1)
    for i, r in enumerate(rows):
        assert i in r and len(r) == m + 1 and np.all(np.diff(r) > 0) and r.min() >= 0 and r.max() < n
        others = np.setdiff1d(np.arange(n), [i])
        best = others[np.lexsort((others, C[i, others]))[:m]]
        assert set(r) == set(best) | {i}
    v = rng.random(n) * C.mean()
    bound = C.mean(axis=1)
    grown, viol = grow(C, rows, v, bound, m)
    gained = 0
    for i, (old, new) in enumerate(zip(rows, grown)):
        assert np.all(np.diff(new) > 0) and set(old) <= set(new) and len(new) - len(old) <= m
        absent = np.setdiff1d(np.arange(n), old)
        below = absent[(C[i, absent] - v[absent]) < bound[i]]
        assert len(new) - len(old) == min(m, below.size) and set(new) - set(old) <= set(below)
        gained += below.size
    assert gained == viol
    cc, ii, kk = to_csr(C, grown)
    assert ii[0] == 0 and ii[-1] == len(cc) == len(kk) and np.array_equal(cc, C[np.repeat(np.arange(n), np.diff(ii)), kk])
    # ties go to the lower column
    rows_c, _ = grow(np.full((9, 9), 3.0), [np.array([i]) for i in range(9)], None, None, 3)
    assert [r.tolist() for r in rows_c[:2]] == [[0, 1, 2, 3], [0, 1, 2, 3]] and rows_c[8].tolist() == [0, 1, 2, 8]
