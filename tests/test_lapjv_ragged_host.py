"""The cold solve of a ragged batch without a GPU: the ABI surface of lapwarm_lapjv_ragged and
lapwarm_lapjv_extended_ragged, the grouping of instances by the kernel configuration of their cold plan
(lapwarm_lapjv_ragged_groups, host only) against the planner's own per-size functions, the workspace queries,
the argument errors, which return before any device work, and the exceptions of `lap.lapjv_many`."""
import ctypes as ct

import numpy as np
import pytest

from host_common import lib  # noqa: F401
from solve_plan_common import plan_solve

ONE_LAUNCH, COLD = 0, 1  # SolveShape::kOneLaunch, kModeCold
INF = float("inf")
NONSQUARE = "Square cost array expected. If cost is intentionally non-square, pass extend_cost=True."


def lapjv_groups_of(lib, sizes):
    arr = (ct.c_int * len(sizes))(*sizes)
    out = (ct.c_int * len(sizes))(*([-7] * len(sizes)))
    return lib.lapwarm_lapjv_ragged_groups(arr, len(sizes), out), list(out)


def cold_plan_queries(lib):
    """-> eligible(n), config(n) from the planner's own per-size functions: plan_solve (cold, no hint, no
    lists) and arr_lists_enabled."""
    plan = plan_solve(lib)
    lists = lib._ZN7lapwarm17arr_lists_enabledEi
    lists.restype, lists.argtypes = ct.c_bool, [ct.c_int]

    def eligible(n):  # one launch, LDS level 2 (prep.ldsl), no helper, no candidate lists
        p = plan(COLD, 1, n, 0, False, 256)
        return p[0] == ONE_LAUNCH and p[3] == 2 and p[13] == 0 and not lists(n)

    def config(n):  # prep: threads, ch, ldsl, tb, lists
        return tuple(plan(COLD, 1, n, 0, False, 256)[1:6])
    return eligible, config, lists


def test_groups_are_the_classes_of_equal_cold_plan_configuration(lib):
    eligible, config, lists = cold_plan_queries(lib)
    first_lists = next(n for n in range(1, 16385) if lists(n))
    assert first_lists == 512  # (default settings: the suite runs without LAPWARM_* in the environment)
    sizes = list(range(1, first_lists))
    assert all(eligible(n) for n in sizes) and not eligible(first_lists)
    count, group_of = lapjv_groups_of(lib, sizes)
    by_config, by_group = {}, {}
    for n, g in zip(sizes, group_of):
        assert by_config.setdefault(config(n), g) == g, (n, "one configuration in two groups")
        assert by_group.setdefault(g, config(n)) == config(n), (n, "two configurations in one group")
    assert count == len(by_config) == len(by_group) and count >= 4
    first = [group_of.index(g) for g in range(count)]
    assert sorted(by_group) == list(range(count)) and first == sorted(first)  # numbered by first appearance
    count_r, group_r = lapjv_groups_of(lib, sizes[::-1])
    assert count_r == count
    assert len({(a, b) for a, b in zip(group_of, group_r[::-1])}) == count


def test_511_is_the_last_eligible_size_and_512_the_first_with_lists(lib):
    eligible, _, lists = cold_plan_queries(lib)
    assert eligible(511) and not lists(511) and lapjv_groups_of(lib, [511]) == (1, [0])
    assert not eligible(512) and lists(512) and lapjv_groups_of(lib, [512])[0] == -1
    for sizes in ([17, 512, 300], [17, 300, 511, 600], [5000]):
        assert lapjv_groups_of(lib, sizes)[0] == -1, sizes
    assert lapjv_groups_of(lib, [17, 100, 200, 300, 511]) == (4, [0, 1, 2, 3, 3])  # 64, 128, 256 and 512 threads
    for n in (0, -3, 16385):
        assert lapjv_groups_of(lib, [17, n])[0] == -1, n
    one = (ct.c_int * 1)(5)
    assert lib.lapwarm_lapjv_ragged_groups(one, 0, one) == -2
    assert lib.lapwarm_lapjv_ragged_groups(None, 1, one) == -2 and lib.lapwarm_lapjv_ragged_groups(one, 1, None) == -2


def _ext_query(lib, rows, cols, limits, extend_cost=1, batch=None):
    B = len(rows)
    return lib.lapwarm_lapjv_extended_ragged_workspace_bytes(
        (ct.c_int * B)(*rows), (ct.c_int * B)(*cols), (ct.c_double * B)(*limits), extend_cost,
        B if batch is None else batch)


def test_workspace_queries(lib):
    q = lib.lapwarm_lapjv_ragged_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(-1, 64) == 0 and q(4, -1) == 0 and q(1, 16385) == 0
    assert q(65536, 8) == 0 and q(1, 1) > 0 and q(65535, 511) >= q(1, 1)
    # extended: 0 for what the call refuses on its arguments
    assert _ext_query(lib, [3], [4], [INF], extend_cost=0) == 0       # non-square without extend_cost
    assert _ext_query(lib, [0], [4], [INF]) == 0 and _ext_query(lib, [4], [-1], [1.0]) == 0
    assert _ext_query(lib, [9000], [9000], [1.0]) == 0                # n = 18000
    assert _ext_query(lib, [3], [4], [INF], batch=0) == 0
    assert lib.lapwarm_lapjv_extended_ragged_workspace_bytes(None, None, None, 1, 1) == 0
    # monotone in the sum of n_b^2, and that sum (not B * N^2) is what it pays for E
    shapes = [(20, 30, INF), (20, 30, 1.0), (100, 100, INF), (100, 100, 0.5), (200, 150, 0.5)]
    got, ssq = [], []
    for k in range(1, len(shapes) + 1):
        rows, cols, lims = zip(*shapes[:k])
        got.append(_ext_query(lib, rows, cols, lims))
        ssq.append(sum((r + c if t < INF else max(r, c)) ** 2 for r, c, t in shapes[:k]))
    assert all(a < b for a, b in zip(got, got[1:])), got
    B, N, R = len(shapes), 350, 200
    fixed = 8 * ssq[-1] + 2 * 8 * B * N + 8 * B * R + 12 * B  # E, the solver's x and y, the matched costs, shapes
    assert fixed <= got[-1] <= fixed + 6 * 256, (fixed, got[-1])
    many_small = _ext_query(lib, [10] * 64 + [250], [10] * 64 + [250], [1.0] * 65)
    assert many_small < 8 * (64 * 20 * 20 + 500 * 500) + 2 * 8 * 65 * 500 + 8 * 65 * 250 + 12 * 65 + 6 * 256


def test_square_argument_errors_return_before_any_device_work(lib):
    """Every call below fails on its arguments alone.  The device pointers are made-up addresses that nothing
    may dereference, and without a GPU any device work would come back as a HIP error (<= -1000)."""
    call = lib.lapwarm_lapjv_ragged
    dev = 1 << 20  # never dereferenced
    host_sizes = (ct.c_int * 3)(5, 64, 300)
    ws_bytes = lib.lapwarm_lapjv_ragged_workspace_bytes(3, 300)
    good = dict(C=dev, offsets=dev, sizes=dev, host_sizes=host_sizes, ld=0, batch=3, N=300, x=dev, y=dev, ret=dev,
                stats=None, ws=dev, ws_bytes=ws_bytes, stream=None)

    def rc(**change):
        a = dict(good, **change)
        return call(a["C"], a["offsets"], a["sizes"], a["host_sizes"], a["ld"], a["batch"], a["N"], a["x"], a["y"],
                    a["ret"], a["stats"], a["ws"], a["ws_bytes"], a["stream"])

    assert rc(batch=0) == -2 and rc(batch=-1) == -2 and rc(batch=65536) == -2
    assert rc(N=0) == -2 and rc(N=-5) == -2 and rc(ld=-1) == -2
    assert rc(N=16385) == -5
    for name in ("C", "offsets", "sizes", "host_sizes", "x", "y", "ret", "ws"):
        assert rc(**{name: None}) == -2, name
    assert rc(N=299) == -2 and rc(ld=200) == -2
    assert rc(host_sizes=(ct.c_int * 3)(5, 0, 300)) == -2
    assert rc(host_sizes=(ct.c_int * 3)(5, 64, 512), N=512) == -6  # outside the class: candidate lists
    assert rc(host_sizes=(ct.c_int * 3)(5, 64, 511), N=511, ws_bytes=ws_bytes - 1) == -1
    assert rc(ws_bytes=0) == -1


def test_extended_argument_errors_return_before_any_device_work(lib):
    call = lib.lapwarm_lapjv_extended_ragged
    dev = 1 << 20  # never dereferenced, 16-byte aligned
    rows, cols, lims = [20, 64, 100], [30, 64, 80], [1.0, INF, 0.5]
    ws_bytes = _ext_query(lib, rows, cols, lims)
    assert ws_bytes > 0

    def arr(t, v):
        return (t * len(v))(*v)
    good = dict(C=dev, offsets=dev, n_rows=dev, n_cols=dev, limit=dev, rows=rows, cols=cols, lims=lims, ld=0, ext=1,
                batch=3, R=100, Q=80, x=dev, y=dev, opt=None, matched=None, ret=dev, stats=None, ws=dev,
                ws_bytes=ws_bytes, stream=None)

    def rc(**change):
        a = dict(good, **change)
        hr = arr(ct.c_int, a["rows"]) if a["rows"] is not None else None
        hc = arr(ct.c_int, a["cols"]) if a["cols"] is not None else None
        hl = arr(ct.c_double, a["lims"]) if a["lims"] is not None else None
        return call(a["C"], a["offsets"], a["n_rows"], a["n_cols"], a["limit"], hr, hc, hl, a["ld"], a["ext"],
                    a["batch"], a["R"], a["Q"], a["x"], a["y"], a["opt"], a["matched"], a["ret"], a["stats"], a["ws"],
                    a["ws_bytes"], a["stream"])

    assert rc(batch=0) == -2 and rc(batch=-3) == -2 and rc(batch=65536) == -2          # empty batch
    assert rc(rows=[20, 0, 100]) == -2 and rc(cols=[30, 64, -1]) == -2                  # empty shape
    for name in ("C", "offsets", "n_rows", "n_cols", "limit", "rows", "cols", "lims", "x", "y", "ret", "ws"):
        assert rc(**{name: None}) == -2, name                                           # bad pointer
    assert rc(ws=dev + 8) == -2                                                         # not 16-byte aligned
    assert rc(R=99) == -2 and rc(Q=79) == -2 and rc(ld=-1) == -2 and rc(ld=70) == -2
    assert rc(ext=0) == -4                                                              # 20 x 30 without extend_cost
    assert rc(rows=[20, 64, 16000], cols=[30, 64, 385], R=16000, Q=385) == -5           # n = 16385
    assert rc(rows=[20, 64, 16385], R=16385, lims=[1.0, INF, INF]) == -5
    assert rc(rows=[20, 64, 300], cols=[30, 64, 300], R=300, Q=300) == -6               # n = 600
    assert rc(rows=[20, 512, 100], cols=[30, 512, 80], R=512, Q=512) == -6              # square 512, no limit
    assert rc(ws_bytes=ws_bytes - 1) == -1 and rc(ws_bytes=0) == -1


def test_lapjv_many_raises_the_reference_messages_before_the_device_is_required():
    import lap
    assert callable(lap.lapjv_many) and "lapjv_many" not in lap.__all__
    ok = np.zeros((3, 3))
    for bad in (np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match="2-dimensional array expected"):
            lap.lapjv_many([ok, bad], extend_cost=True)
    for limit in (INF, 1.0):
        with pytest.raises(ValueError) as e:
            lap.lapjv_many([ok, np.zeros((3, 2))], cost_limit=limit)
        assert str(e.value) == NONSQUARE
    with pytest.raises(TypeError):
        lap.lapjv_many([ok, None])
    with pytest.raises(TypeError):
        lap.lapjv_many([ok], cost_limit="a lot")
    with pytest.raises(ValueError, match="cost limits"):
        lap.lapjv_many([ok, ok], cost_limit=[1.0])
    # nothing to match: answered as lap.lapjv_extended does, without a device
    out = lap.lapjv_many([np.zeros((0, 5)), np.zeros((4, 0))], extend_cost=True, cost_limit=[INF, 2.0])
    assert out[0][0] == 0.0 and out[0][1].shape == (0,) and list(out[0][2]) == [-1] * 5
    assert list(out[1][1]) == [-1] * 4 and out[1][2].shape == (0,) and out[1][1].dtype == np.int32
    assert lap.lapjv_many([]) == []
