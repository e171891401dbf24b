"""CPU tests of the rectangular / cost-limited lapjv: the four C symbols are declared and exported,
lapwarm_lapjv_extended_n (which needs no device) restates _lapjv.pyx:77-95, `lap.lapjv_extended` raises the
reference's exceptions before any device work, `lap.lapjv` still refuses the two arguments, and the CPU
oracle on the numpy-built extended matrix reproduces every fixture of the reference build
(tests/golden/lapjv_extended_cases.npz), so that it can stand in for the reference at larger sizes."""
import re
from pathlib import Path

import numpy as np
import pytest

from host_common import lib_or_skip as lib  # noqa: F401
from lapjv_extended_common import ExtendedCases, assert_case, build_E, extended_n, solve_with

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("lapwarm_lapjv_extended", "lapwarm_lapjv_extended_n", "lapwarm_lapjv_extended_workspace_bytes",
           "lapwarm_lapjv_extended_batched")
INF = float("inf")
NONSQUARE = "Square cost array expected. If cost is intentionally non-square, pass extend_cost=True."


def test_header_declares_the_four_symbols():
    header = (ROOT / "include" / "lapwarm_hip.h").read_text()
    declared = set(re.findall(r"\b(lapwarm_\w+)\s*\(", header))
    assert set(SYMBOLS) <= declared, set(SYMBOLS) - declared


def test_library_exports_the_four_symbols(lib):
    from lap import _hip
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES, name


@pytest.mark.parametrize("n_rows,n_cols,extend_cost,limit,want", [
    (3, 3, 0, INF, 3), (3, 3, 1, INF, 3), (3, 3, 0, 4.99, 6), (3, 3, 1, 4.99, 6),
    (2, 4, 1, INF, 4), (4, 2, 1, INF, 4), (2, 4, 1, 10.0, 6), (7, 3, 1, 0.0, 10), (7, 3, 1, -1.0, 10),
    (1, 9, 1, INF, 9), (11, 1, 1, 5.0, 12), (255, 256, 1, 0.02, 511), (2300, 2300, 0, 0.01, 4600),
    (2, 4, 0, INF, -4), (2, 4, 0, 10.0, -4), (4, 2, 0, 0.5, -4),
    (0, 4, 1, INF, -2), (4, 0, 1, 1.0, -2), (-1, 4, 1, INF, -2), (0, 0, 0, INF, -2), (0, 4, 0, INF, -2),
    (16384, 16384, 0, INF, 16384), (16384, 5, 1, INF, 16384), (16385, 5, 1, INF, -5), (5, 16385, 1, INF, -5),
    (8192, 8192, 0, 1.0, 16384), (8192, 8193, 1, 1.0, -5), (16384, 16384, 1, 1e300, -5),
    (2147483647, 2147483647, 0, 1.0, -5),
    (3, 3, 0, float("nan"), 3), (2, 4, 1, float("nan"), 4),  # `cost_limit < np.inf` is false for NaN
])
def test_extended_n_table(lib, n_rows, n_cols, extend_cost, limit, want):
    assert lib.lapwarm_lapjv_extended_n(n_rows, n_cols, extend_cost, limit) == want
    if want > 0:
        assert want == extended_n(n_rows, n_cols, extend_cost, limit)


def test_workspace_bytes(lib):
    q = lib.lapwarm_lapjv_extended_workspace_bytes
    cold = lib.lapwarm_lapjv_workspace_bytes
    for B, r, c, ext, lim in ((1, 1024, 1024, 0, 0.01), (32, 2048, 1024, 1, INF), (3, 255, 256, 1, 0.02), (2, 1, 9, 1, INF)):
        n = extended_n(r, c, ext, lim)
        fixed = 8 * B * n * n + 2 * 4 * B * n + 8 * B * r + cold(B, n)  # E, the solver's x and y, the matched costs
        assert fixed <= q(B, r, c, ext, lim) <= fixed + 5 * 256, (B, r, c)
    # a square matrix without a limit is solved where it is: no E
    assert q(4, 300, 300, 1, INF) < cold(4, 300) + 4 * 300 * 16 + 5 * 256
    for bad in ((1, 3, 4, 0, INF), (0, 3, 3, 1, INF), (1, 0, 3, 1, INF), (1, 9000, 9000, 0, 1.0)):
        assert q(*bad) == 0, bad


def test_argument_errors_come_before_device_work():
    import lap
    with pytest.raises(TypeError):
        lap.lapjv_extended(None)
    for bad in (np.zeros(3), np.zeros((2, 2, 2)), np.ndarray([])):
        with pytest.raises(ValueError, match="2-dimensional array expected"):
            lap.lapjv_extended(bad, extend_cost=True)
    for limit in (INF, 1.0):
        with pytest.raises(ValueError) as e:
            lap.lapjv_extended(np.zeros((3, 2)), cost_limit=limit)
        assert str(e.value) == NONSQUARE
    with pytest.raises(TypeError):
        lap.lapjv_extended(np.zeros((2, 2)), cost_limit="a lot")


def test_empty_inputs_do_not_touch_the_device():
    import lap
    opt, x, y = lap.lapjv_extended(np.zeros((0, 5)), extend_cost=True)
    assert opt == 0.0 and x.shape == (0,) and list(y) == [-1] * 5 and x.dtype == y.dtype == np.int32
    opt, x, y = lap.lapjv_extended(np.zeros((4, 0)), extend_cost=True, cost_limit=2.0)
    assert opt == 0.0 and list(x) == [-1] * 4 and y.shape == (0,)
    x, y = lap.lapjv_extended(np.zeros((0, 0)), cost_limit=2.0, return_cost=False)
    assert x.shape == y.shape == (0,)


def test_no_device_means_loud_failure(lib):
    import lap
    if lib.lapwarm_device_count() > 0:
        pytest.skip("GPU present")
    for kw in (dict(extend_cost=True), dict(cost_limit=1.0), dict()):
        with pytest.raises(RuntimeError, match="no HIP device"):
            lap.lapjv_extended(np.zeros((4, 4)), **kw)


def test_lapjv_keeps_refusing_and_all_is_unchanged():
    import lap
    with pytest.raises(NotImplementedError, match="lap.lapjv_extended"):
        lap.lapjv(np.zeros((3, 4)), extend_cost=True)
    with pytest.raises(NotImplementedError, match="lap.lapjv_extended"):
        lap.lapjv(np.zeros((3, 3)), cost_limit=0.5)
    assert callable(lap.lapjv_extended) and "lapjv_extended" not in lap.__all__
    assert "lapjv_extended" in lap.__doc__ and "__all__" in lap.__doc__


def test_fixture_file_covers_what_it_should():
    cases = ExtendedCases()
    assert 40 <= len(cases) <= 120 and (ROOT / "tests" / "golden" / "lapjv_extended_cases.npz").stat().st_size < 1 << 20
    metas = [cases.case(k) for k in range(len(cases))]
    shapes = {(m["n_rows"], m["n_cols"]) for m in metas}
    assert any(r > c > 1 for r, c in shapes) and any(1 < r < c for r, c in shapes) and any(r == c > 1 for r, c in shapes)
    assert any(r == 1 < c for r, c in shapes) and any(c == 1 < r for r, c in shapes)
    limited = [m for m in metas if m["cost_limit"] < np.inf]
    assert any(m["cost_limit"] < m["C"].min() and (m["x"] == -1).all() for m in limited)       # below every entry
    assert any(m["cost_limit"] > m["C"].max() for m in limited)                                 # above every entry
    assert any(0 < (m["x"] != -1).sum() < min(m["C"].shape) for m in limited)                   # between entries
    assert any(not m["extend_cost"] for m in limited) and any(m["cost_limit"] == np.inf for m in metas)
    by = {m["label"]: m for m in metas}
    k = by["known_extension_2x4"]   # LAP/lap/tests/test_lapjv.py:34-39
    assert k["opt"] == 3.0 and list(k["x"]) == [1, 2] and list(k["y"]) == [-1, 0, 1, -1]
    k = by["known_cost_limit_3x3"]  # test_lapjv.py:52-57
    assert k["opt"] == 3.0 and list(k["x"]) == [1, 2, -1] and list(k["y"]) == [-1, 0, 1] and k["cost_limit"] == 4.99
    k = by["known_arr_loop_7x3"]    # test_arr_loop.py:45-60
    assert abs(k["opt"] - 0.8455356917416) <= 1e-10 * 0.8455356917416
    assert sorted([list(k["y"]), list(k["y_alt"])]) == [[1, 5, 2], [5, 1, 2]]


CASES = ExtendedCases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASES.labels)
def test_oracle_reproduces_fixture(k):
    """oracle.jv.dense_raw on E built by numpy, then _lapjv.pyx:116-122: the reference build's opt, x, y."""
    from oracle import jv
    c = CASES.case(k)
    E = build_E(c["C"], c["extend_cost"], c["cost_limit"])
    n = extended_n(c["n_rows"], c["n_cols"], c["extend_cost"], c["cost_limit"])
    assert E.shape == (n, n) and E.flags.c_contiguous
    opt, x, y, _ = solve_with(jv.dense_raw, c["C"], c["extend_cost"], c["cost_limit"])
    assert_case(c, opt, x, y)
