"""The seeded solve of a ragged batch without a GPU: the ABI surface of lapwarm_seeded_ragged, the grouping of
instances by kernel configuration (lapwarm_seeded_ragged_groups, host only) against the per-size plan queries
the library exports, the workspace query, and the argument errors, which return before any device work."""
import ctypes as ct

import pytest

from host_common import lib  # noqa: F401
from solve_plan_common import plan_solve

ONE_LAUNCH = 0  # SolveShape::kOneLaunch


def seeded_groups_of(lib, sizes):
    arr = (ct.c_int * len(sizes))(*sizes)
    out = (ct.c_int * len(sizes))(*([-7] * len(sizes)))
    return lib.lapwarm_seeded_ragged_groups(arr, len(sizes), out), list(out)


def seeded_plan_queries(lib):
    """-> eligible(n), config(n) from the planner's own per-size functions: plan_solve (seeded, no hint, no
    lists), solver_uses_helpers and solver_needs_global_state."""
    plan = plan_solve(lib)
    helpers, global_state = lib._ZN7lapwarm19solver_uses_helpersEi, lib._ZN7lapwarm25solver_needs_global_stateEi
    for f in (helpers, global_state):
        f.restype, f.argtypes = ct.c_bool, [ct.c_int]

    def eligible(n):
        return plan(0, 1, n, 0, False, 256)[0] == ONE_LAUNCH and not helpers(n) and not global_state(n)

    def config(n):  # prep: threads, ch, ldsl, tb, lists
        return tuple(plan(0, 1, n, 0, False, 256)[1:6])
    return eligible, config


def test_groups_are_the_classes_of_equal_plan_configuration(lib):
    eligible, config = seeded_plan_queries(lib)
    sizes = [n for n in range(1, 1101) if eligible(n)]
    # every size below the first helper size, and the odd ones above it
    assert [n for n in range(1, 1101) if n not in sizes] == list(range(1024, 1101, 2))
    count, group_of = seeded_groups_of(lib, sizes)
    by_config, by_group = {}, {}
    for n, g in zip(sizes, group_of):
        assert by_config.setdefault(config(n), g) == g, (n, "one configuration in two groups")
        assert by_group.setdefault(g, config(n)) == config(n), (n, "two configurations in one group")
    assert count == len(by_config) == len(by_group) and count >= 5
    first = [group_of.index(g) for g in range(count)]
    assert sorted(by_group) == list(range(count)) and first == sorted(first)  # numbered by first appearance
    # the same classes whatever the order of the instances
    count_r, group_r = seeded_groups_of(lib, sizes[::-1])
    assert count_r == count
    assert len({(a, b) for a, b in zip(group_of, group_r[::-1])}) == count


@pytest.mark.parametrize("bad", (1024, 5000))
def test_one_ineligible_size_makes_the_whole_list_ineligible(lib, bad):
    eligible, _ = seeded_plan_queries(lib)
    assert not eligible(bad)
    assert seeded_groups_of(lib, [17, 300, 1023])[0] == 3  # 64, 512 and 1024 threads
    for sizes in ([bad], [17, bad, 300], [17, 300, 1023, bad]):
        assert seeded_groups_of(lib, sizes)[0] == -1, sizes
    for n in (0, -3, 16385):
        assert seeded_groups_of(lib, [17, n])[0] == -1, n
    one = (ct.c_int * 1)(5)
    assert lib.lapwarm_seeded_ragged_groups(one, 0, one) == -2
    assert lib.lapwarm_seeded_ragged_groups(None, 1, one) == -2 and lib.lapwarm_seeded_ragged_groups(one, 1, None) == -2


def test_workspace_query_is_monotone_and_zero_for_invalid_dimensions(lib):
    q = lib.lapwarm_seeded_ragged_workspace_bytes
    assert q(1, 0) == 0 and q(0, 64) == 0 and q(-1, 64) == 0 and q(4, -1) == 0
    assert q(1, 16385) == 0 and q(65536, 8) == 0
    batches = (1, 2, 3, 7, 32, 33, 1000, 65535)
    widths = (1, 2, 31, 32, 33, 512, 513, 1023, 2047, 3633)
    for N in widths:
        got = [q(B, N) for B in batches]
        # three fp64 and two int32 per padded row, and the tight-edge bitmap
        assert got[0] >= N * (3 * 8 + 2 * 4) + N * ((N + 31) // 32) * 4, (N, got[0])
        assert all(a <= b for a, b in zip(got, got[1:])) and got[0] < got[-1], (N, got)  # (256-byte granules)
    for B in batches:
        got = [q(B, N) for N in widths]
        assert all(a <= b for a, b in zip(got, got[1:])), (B, got)


def test_argument_errors_return_before_any_device_work(lib):
    """Every call below fails on its arguments alone.  The device pointers are made-up addresses that nothing
    may dereference, and without a GPU any device work would come back as a HIP error (<= -1000)."""
    call = lib.lapwarm_seeded_ragged
    dev = 1 << 20  # never dereferenced
    host_sizes = (ct.c_int * 3)(5, 64, 300)
    ws_bytes = lib.lapwarm_seeded_ragged_workspace_bytes(3, 300)
    good = dict(C=dev, offsets=dev, sizes=dev, host_sizes=host_sizes, ld=0, batch=3, N=300, u=dev, v=dev, eps=1e-12,
                x=dev, y=dev, ret=dev, stats=None, ws=dev, ws_bytes=ws_bytes, stream=None)

    def rc(**change):
        a = dict(good, **change)
        return call(a["C"], a["offsets"], a["sizes"], a["host_sizes"], a["ld"], a["batch"], a["N"], a["u"], a["v"],
                    a["eps"], a["x"], a["y"], a["ret"], a["stats"], a["ws"], a["ws_bytes"], a["stream"])

    assert rc(batch=0) == -2 and rc(batch=-1) == -2 and rc(batch=65536) == -2
    assert rc(N=0) == -2 and rc(N=-5) == -2 and rc(ld=-1) == -2
    assert rc(N=16385) == -5
    for name in ("C", "offsets", "sizes", "host_sizes", "u", "v", "x", "y", "ret", "ws"):
        assert rc(**{name: None}) == -2, name
    assert rc(N=299) == -2  # a size above the padded width
    assert rc(ld=200) == -2  # ... or above the row stride
    assert rc(host_sizes=(ct.c_int * 3)(5, 0, 300)) == -2
    assert rc(host_sizes=(ct.c_int * 3)(5, 64, 1024), N=1024) == -6  # outside the class: helper workgroups
    assert rc(ws_bytes=ws_bytes - 1) == -1
