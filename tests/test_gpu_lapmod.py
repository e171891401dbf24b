"""Sparse LAPMOD on the MI355X against the reference's lapmod_internal (tests/golden/lapmod_cases.npz and
lapmod_long_rows.npz): every case for FP_1, FP_2 and FP_DYNAMIC through `lap.lapmod_sparse`, `lap.lapmod_many` and
`WarmStartPipeline.lapmod_ragged`, the final duals, the dense solver on the densified matrix, the stats, the LDS /
workspace boundary, an unsolvable instance inside a batch, rows of two to four wave-loads with inexact costs in the
search, input that only the kernel's own check can reject, the workspace plan across a chunk of 64 instances, graph
capture, and `solvers.LAPMODSolver`."""
import numpy as np
import pytest

from host_common import shared_pipe as pipe  # noqa: F401
from lapmod_common import FP_VERSIONS, densify, load_cases, long_row_labels, problem

pytestmark = pytest.mark.gpu

CASES, LDS_MAX = load_cases()
LABELS = list(CASES)
LONG = long_row_labels()


def expect(c, fp, opt, x, y, label):
    """What a device result must be, from the fixture."""
    import lap
    n = c["n"]
    if c["solvable"]:
        ret, rx, ry = c["ref"][fp]
        assert ret == 0
        assert np.array_equal(x, rx) and np.array_equal(y, ry), (label, fp)
        assert opt == lap.get_cost(*problem(c), rx) and np.isfinite(opt), (label, fp)
    else:
        assert opt == np.inf, (label, fp)
        unmatched = np.array_equal(x, np.full(n, -1)) and np.array_equal(y, np.full(n, -1))
        if c["strict"]:
            assert unmatched, (label, fp)
        elif not unmatched and fp in c["ref"]:  # neither condition of `ret = 1` was met: the reference's result
            assert np.array_equal(x, c["ref"][fp][1]) and np.array_equal(y, c["ref"][fp][2]), (label, fp)
    assert x.dtype == np.int32 and y.dtype == np.int32 and x.shape == (n,) and y.shape == (n,)


@pytest.fixture(scope="module")
def singles():
    """(label, fp) -> (opt, x, y) of lapmod_sparse, computed once."""
    import lap
    return {(label, fp): lap.lapmod_sparse(*problem(CASES[label]), fp_version=fp)
            for label in LABELS for fp in FP_VERSIONS}


@pytest.fixture(scope="module")
def ragged(pipe):
    """fp -> the padded result of one lapmod_ragged call over every case, on the host."""
    import torch
    from gnn.pipeline import sparse_pack
    pack = sparse_pack([problem(CASES[label]) for label in LABELS], pipe.device)
    out = {}
    for fp in FP_VERSIONS:
        r = pipe.lapmod_ragged(pack, fp, want_stats=True)
        torch.cuda.synchronize()
        out[fp] = {k: t.cpu().numpy() for k, t in r.items()}
    return out


@pytest.mark.parametrize("fp", FP_VERSIONS)
def test_every_case_matches_the_reference(singles, fp):
    for label in LABELS:
        opt, x, y = singles[(label, fp)]
        expect(CASES[label], fp, opt, x, y, label)


def test_fast_false_and_return_cost_false(singles):
    import lap
    c = CASES["n65_sparse_tie"]
    for fp in FP_VERSIONS:
        opt, x, y = singles[("n65_sparse_tie", fp)]
        o2, x2, y2 = lap.lapmod_sparse(*problem(c), fast=False, fp_version=fp)
        assert o2 == opt and np.array_equal(x2, x) and np.array_equal(y2, y)
        x3, y3 = lap.lapmod_sparse(*problem(c), return_cost=False, fp_version=fp)
        assert np.array_equal(x3, x) and np.array_equal(y3, y)


@pytest.mark.parametrize("fp", FP_VERSIONS)
def test_many_in_shuffled_order_equals_the_single_calls(singles, fp):
    import lap
    order = np.random.default_rng(5).permutation(len(LABELS))
    got = lap.lapmod_many([problem(CASES[LABELS[k]]) for k in order], fp_version=fp)
    assert len(got) == len(LABELS)
    for k, (opt, x, y) in zip(order, got):
        so, sx, sy = singles[(LABELS[k], fp)]
        assert opt == so and np.array_equal(x, sx) and np.array_equal(y, sy), (LABELS[k], fp)
    pairs = lap.lapmod_many([problem(CASES[LABELS[k]]) for k in order[:5]], fp_version=fp, return_cost=False)
    assert all(len(p) == 2 for p in pairs)


@pytest.mark.parametrize("fp", FP_VERSIONS)
def test_ragged_ret_padding_and_rows(ragged, singles, fp):
    r = ragged[fp]
    N = max(c["n"] for c in CASES.values())
    assert r["x"].shape == (len(LABELS), N) and r["v"].shape == (len(LABELS), N)
    for b, label in enumerate(LABELS):
        c, n = CASES[label], CASES[label]["n"]
        _, sx, sy = singles[(label, fp)]
        assert np.array_equal(r["x"][b, :n], sx) and np.array_equal(r["y"][b, :n], sy), (label, fp)
        assert np.all(r["x"][b, n:] == -1) and np.all(r["y"][b, n:] == -1) and np.all(np.isnan(r["v"][b, n:]))
        if c["solvable"]:
            assert r["ret"][b] == 0, (label, fp)
        elif c["strict"]:
            assert r["ret"][b] == 1, (label, fp)
        else:
            assert r["ret"][b] in (0, 1), (label, fp)
        if r["ret"][b] != 0:
            assert np.all(r["x"][b] == -1) and np.all(np.isnan(r["v"][b]))


@pytest.mark.parametrize("fp", FP_VERSIONS)
def test_final_duals_equal_the_reference_bit_for_bit(ragged, fp):
    """v of every solvable case has the bit patterns of the reference's final v (0 ulp, no tolerance).  With that,
    feasibility and tightness are those of the reference's arithmetic: u_i = c[i, x_i] - v[x_i] is the smallest
    c - v[j] of row i.  Integer costs make every operation exact, so the slack is >= 0 there without any bound;
    with continuous costs the slack of the device's v is the slack of the reference's, element for element."""
    r = ragged[fp]
    checked = 0
    for b, label in enumerate(LABELS):
        c, n = CASES[label], CASES[label]["n"]
        if not c["solvable"]:
            continue
        v, x = r["v"][b, :n], r["x"][b, :n]
        ref_v = c["v"][fp]
        assert np.array_equal(v.view(np.int64), ref_v.view(np.int64)), (label, fp, np.abs(v - ref_v).max())
        rows = np.repeat(np.arange(n), np.diff(c["ii"]))
        on_match = c["kk"] == x[rows]
        assert on_match.sum() == n, label

        def slack(duals):
            red = c["cc"] - duals[c["kk"]]
            u = np.empty(n)
            u[rows[on_match]] = red[on_match]
            return red - u[rows]

        got = slack(v)
        assert np.all(got[on_match] == 0.0), label
        if np.all(c["cc"] == np.floor(c["cc"])):
            assert np.all(got >= 0.0), (label, fp, got.min())
        else:
            assert np.array_equal(got, slack(ref_v)), (label, fp)
        checked += 1
    assert checked == 49  # every solvable case


def test_cost_equals_the_dense_solver(singles):
    """Every solvable case, the LDS boundary and n = 4096 included, against lap.lapjv on the densified matrix
    (absent = 1e5).  Both costs are summed row by row, left to right, over the same entries: equal, not close."""
    import lap
    for label in LABELS:
        c = CASES[label]
        if not c["solvable"]:
            continue
        dense_x = lap.lapjv(densify(c, absent=1e5))[1]
        dense_opt = lap.get_cost(*problem(c), dense_x)
        assert np.isfinite(dense_opt), label
        for fp in FP_VERSIONS:
            assert singles[(label, fp)][0] == dense_opt, (label, fp)


def test_stats_name_the_search_that_ran(ragged):
    r = ragged[3]["stats"]
    seen = set()
    for b, label in enumerate(LABELS):
        c = CASES[label]
        if not c["solvable"]:
            continue
        assert r[b, 8] == c["n"] and r[b, 9] == c["ii"][-1] and r[b, 11] == c["dyn"], label
        assert r[b, 7] == (c["dyn"] if c["aug"] else 0), label
        assert (r[b, 4] > 0) == c["aug"] and (r[b, 5] > 0) == c["aug"], label
        assert r[b, 0] >= max(r[b, 1], 0) or r[b, 1] == -1
        if c["aug"]:
            seen.add(c["dyn"])
    assert seen == {1, 2}
    for fp in (1, 2):
        s = ragged[fp]["stats"]
        for b, label in enumerate(LABELS):
            if CASES[label]["solvable"] and CASES[label]["aug"]:
                assert s[b, 7] == fp and s[b, 11] == fp, label


def test_lds_and_workspace_sides_of_the_boundary(ragged, singles):
    below, above = f"n{LDS_MAX}_lds_bound", f"n{LDS_MAX + 1}_above_lds"
    s = ragged[2]["stats"]
    assert s[LABELS.index(below), 10] == 1 and s[LABELS.index(above), 10] == 0
    assert s[LABELS.index("n4096_k16"), 10] == 0 and s[LABELS.index("n1_dense_int"), 10] == 1
    for label in (below, above, "n4096_k16"):
        for fp in FP_VERSIONS:
            expect(CASES[label], fp, *singles[(label, fp)], label)


def test_unsolvable_instance_leaves_its_neighbours_intact(pipe, singles):
    import lap
    labels = ["n64_sparse_tie", "empty_column", "n63_dense_tie", "infs_unsolvable1", "known8_masked"]
    for fp in FP_VERSIONS:
        got = lap.lapmod_many([problem(CASES[label]) for label in labels], fp_version=fp)
        for label, (opt, x, y) in zip(labels, got):
            so, sx, sy = singles[(label, fp)]
            assert opt == so and np.array_equal(x, sx) and np.array_equal(y, sy), (label, fp)
        assert got[1][0] == np.inf and np.all(got[1][1] == -1) and np.all(got[3][2] == -1)
        assert np.isfinite(got[0][0]) and np.isfinite(got[2][0]) and got[4][0] == 17.0


def test_long_rows_reach_the_search_they_were_given(ragged):
    """The cases of lapmod_long_rows.npz (rows of 64 to 193 entries, costs that fp64 rounds): the path search ran
    under every fp_version, and a forced search is the one that ran.  That its x, y and v are the reference's is what
    the tests above assert for every label."""
    seen = 0
    for fp in FP_VERSIONS:
        s = ragged[fp]["stats"]
        for label in LONG:
            if not CASES[label]["solvable"]:
                continue
            b = LABELS.index(label)
            print(f"{label} fp={fp}: paths {s[b, 4]}, finds {s[b, 5]}, scan steps {s[b, 6]}, search {s[b, 7]}")
            assert s[b, 4] > 0 and s[b, 5] > 0 and s[b, 6] > 0, (label, fp)
            if fp in (1, 2):
                assert s[b, 7] == fp, (label, fp)
            seen += 1
    assert seen == 3 * 9


def test_unsolvable_long_rows_inside_a_batch(ragged, singles):
    """ret = 1 above n = 64, from an empty column and from two rows that hold one column between them, each between
    two solvable long-row cases of one lapmod_many call."""
    import lap
    labels = ["dec_rows65_n130", "dec_empty_col130", "dec_full193", "dec_hall130", "dec_sparse130"]
    for fp in FP_VERSIONS:
        got = lap.lapmod_many([problem(CASES[label]) for label in labels], fp_version=fp)
        for k in (1, 3):
            opt, x, y = got[k]
            n = CASES[labels[k]]["n"]
            assert opt == np.inf and np.array_equal(x, np.full(n, -1)) and np.array_equal(y, np.full(n, -1)), (k, fp)
            assert ragged[fp]["ret"][LABELS.index(labels[k])] == 1, (labels[k], fp)
        for k in (0, 2, 4):
            so, sx, sy = singles[(labels[k], fp)]
            assert np.isfinite(so) and got[k][0] == so, (labels[k], fp)
            assert np.array_equal(got[k][1], sx) and np.array_equal(got[k][2], sy), (labels[k], fp)


REJECT_LABELS = ["n65_dense_tie", "known8_masked", "n64_sparse_tie", "inf_unique", "n63_sparse_cont"]


def _ragged_host(pipe, pack, fp):
    import torch
    r = pipe.lapmod_ragged(pack, fp, want_stats=True)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in r.items()}


@pytest.fixture(scope="module")
def reject_pack(pipe):
    """The pack of REJECT_LABELS and its clean result under FP_1 and FP_2."""
    from gnn.pipeline import sparse_pack
    pack = sparse_pack([problem(CASES[label]) for label in REJECT_LABELS], pipe.device)
    return pack, {fp: _ragged_host(pipe, pack, fp) for fp in (1, 2)}


def _corrupted(pack):
    """A copy of the pack whose device tensors are its own."""
    from gnn.pipeline import SparsePack
    return SparsePack(pack.cc.clone(), pack.kk.clone(), pack.ii.clone(), pack.nnz_offsets.clone(),
                      pack.row_offsets.clone(), pack.sizes.clone(), list(pack.host_sizes), list(pack.host_nnz))


def _same_as_clean(got, clean, b):
    return (np.array_equal(got["x"][b], clean["x"][b]) and np.array_equal(got["y"][b], clean["y"][b])
            and got["ret"][b] == clean["ret"][b]
            and np.array_equal(got["v"][b].view(np.int64), clean["v"][b].view(np.int64)))


# name -> (what it does to instance b of a pack p: n rows, entries e0 .. e0 + nnz - 1, row starts from r0; targets).
# Entry corruptions hit the instance's last entry and row-start ones its last rows, so that with n >= 64 a later
# turn of the kernel's 64-strided check loops is the one that sees them.  ii[n] is never touched.
def _last_column(value):
    def corrupt(p, b, n, nnz, e0, r0):
        p.kk[e0 + nnz - 1] = n if value == "n" else value
    return corrupt


def _last_cost(value):
    def corrupt(p, b, n, nnz, e0, r0):
        p.cc[e0 + nnz - 1] = value
    return corrupt


def _swap_row_starts(p, b, n, nnz, e0, r0):
    p.ii[r0 + n - 2:r0 + n] = p.ii[r0 + n - 2:r0 + n].flip(0)  # row n - 2 ends before it starts


def _first_row_start_one(p, b, n, nnz, e0, r0):
    p.ii[r0] = 1


def _one_row_holds_everything(p, b, n, nnz, e0, r0):
    p.ii[r0 + 1:r0 + n] = nnz  # ii = [0, nnz, nnz, ..., nnz]


def _size(value):
    def corrupt(p, b, n, nnz, e0, r0):
        p.sizes[b] = max(p.host_sizes) + 1 if value == "N + 1" else value
    return corrupt


FIRST_FOUR = (0, 1, 2, 3)
CORRUPTIONS = {
    "column_n": (_last_column("n"), FIRST_FOUR),
    "column_minus_one": (_last_column(-1), FIRST_FOUR),
    "cost_nan": (_last_cost(float("nan")), FIRST_FOUR),
    "cost_minus_one": (_last_cost(-1.0), FIRST_FOUR),
    "cost_large": (_last_cost(1e6), FIRST_FOUR),
    "cost_inf": (_last_cost(float("inf")), FIRST_FOUR),
    "row_starts_swapped": (_swap_row_starts, FIRST_FOUR),
    "first_row_start_one": (_first_row_start_one, FIRST_FOUR),
    "row_of_316_entries": (_one_row_holds_everything, (REJECT_LABELS.index("n64_sparse_tie"),)),
    "size_zero": (_size(0), FIRST_FOUR),
    "size_above_N": (_size("N + 1"), FIRST_FOUR),
}


@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_device_check_rejects_what_the_host_never_saw(pipe, reject_pack, name):
    """`lapmod_ragged` takes a SparsePack as it is: the kernel's own check is the only guard of its device tensors.
    One instance is corrupted in place on the device (never the last one, every instance has its state in LDS and
    ii[n] stays): ret = 2, x and y -1, v NaN and a zero stats row for it, the clean call's bits for the others."""
    import torch
    pack, clean = reject_pack
    corrupt, targets = CORRUPTIONS[name]
    row0, ent0 = pack.row_offsets.cpu().tolist(), pack.nnz_offsets.cpu().tolist()
    for b in targets:
        n, nnz = pack.host_sizes[b], pack.host_nnz[b]
        assert b < len(REJECT_LABELS) - 1 and n <= LDS_MAX
        bad = _corrupted(pack)
        corrupt(bad, b, n, nnz, ent0[b], row0[b])
        assert int(bad.ii[row0[b] + n]) == nnz == int(pack.ii[row0[b] + n])
        changed = sum(int(torch.sum(getattr(bad, k) != getattr(pack, k))) for k in ("kk", "ii", "sizes"))
        changed += int(torch.sum(bad.cc.view(torch.int64) != pack.cc.view(torch.int64)))
        assert 1 <= changed <= n, (name, b)
        for fp in (2, 1):
            got = _ragged_host(pipe, bad, fp)
            assert got["ret"][b] == 2, (name, b, fp)
            assert np.all(got["x"][b] == -1) and np.all(got["y"][b] == -1), (name, b, fp)
            assert np.all(np.isnan(got["v"][b])) and not np.any(got["stats"][b]), (name, b, fp)
            for other in range(len(REJECT_LABELS)):
                if other != b:
                    assert _same_as_clean(got, clean[fp], other), (name, b, fp, other)
                    assert np.array_equal(got["stats"][other], clean[fp]["stats"][other]), (name, b, fp, other)
        if name == "row_of_316_entries":
            assert int(bad.ii[row0[b] + 1]) - int(bad.ii[row0[b]]) == 316 > n


def test_minus_zero_cost_is_read_as_zero(pipe, reject_pack):
    """DESIGN.md, difference 4: the stored 0.0 of inf_unique overwritten with -0.0 on the device solves to the
    bits of the clean call."""
    import torch
    pack, clean = reject_pack
    b = REJECT_LABELS.index("inf_unique")
    e0 = int(pack.nnz_offsets[b])
    zero = np.flatnonzero(CASES["inf_unique"]["cc"] == 0.0)
    assert zero.size == 1
    neg = _corrupted(pack)
    neg.cc[e0 + int(zero[0])] = -0.0
    assert int(neg.cc.view(torch.int64)[e0 + int(zero[0])]) == -2 ** 63
    for fp in (2, 1):
        got = _ragged_host(pipe, neg, fp)
        assert got["ret"][b] == 0 and np.array_equal(got["x"][b, :4], CASES["inf_unique"]["ref"][fp][1])
        for other in range(len(REJECT_LABELS)):
            assert _same_as_clean(got, clean[fp], other), (fp, other)
            assert np.array_equal(got["stats"][other], clean[fp]["stats"][other]), (fp, other)


def test_workspace_plan_across_a_chunk_of_64_instances(pipe):
    """B = 70 under FP_2 with the above-LDS case at positions 0, 63, 64 and 69 and n = 4096 at 30: the workspace
    offsets need the prefix inside a chunk of 64 and the sum carried into the next one to keep five states apart.
    Every instance equals a call of its own, v bit for bit."""
    import time
    import torch
    from gnn.pipeline import sparse_pack
    above = f"n{LDS_MAX + 1}_above_lds"
    labels = ["known8_masked"] * 70
    for pos in (0, 63, 64, 69):
        labels[pos] = above
    labels[30] = "n4096_k16"
    alone = {label: _ragged_host(pipe, sparse_pack([problem(CASES[label])], pipe.device), 2)
             for label in set(labels)}
    pack = sparse_pack([problem(CASES[label]) for label in labels], pipe.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = _ragged_host(pipe, pack, 2)
    print(f"B = 70 lapmod_ragged call: {time.perf_counter() - t0:.3f} s")
    assert got["x"].shape == (70, 4096)
    for b, label in enumerate(labels):
        n, one = CASES[label]["n"], alone[label]
        assert got["stats"][b, 10] == (0 if n > LDS_MAX else 1), (b, label)
        assert got["ret"][b] == 0 == one["ret"][0], (b, label)
        assert np.array_equal(got["x"][b, :n], one["x"][0]) and np.array_equal(got["y"][b, :n], one["y"][0]), b
        assert np.array_equal(got["x"][b, :n], CASES[label]["ref"][2][1]), (b, label)
        assert np.array_equal(got["v"][b, :n].view(np.int64), one["v"][0].view(np.int64)), (b, label)
        assert np.array_equal(one["v"][0].view(np.int64), CASES[label]["v"][2].view(np.int64)), label
        assert np.all(got["x"][b, n:] == -1) and np.all(np.isnan(got["v"][b, n:])), b


def test_graph_capture_and_replay(pipe):
    import torch
    from gnn.pipeline import sparse_pack
    labels = ["n257_sparse_tie", "empty_column", "n65_dense_tie", f"n{LDS_MAX + 1}_above_lds"]
    pack = sparse_pack([problem(CASES[label]) for label in labels], pipe.device)
    eager = pipe.lapmod_ragged(pack, 2)
    torch.cuda.synchronize()
    want = {k: t.clone() for k, t in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.lapmod_ragged(pack, 2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipe.lapmod_ragged(pack, 2)
    for _ in range(2):
        for t in out.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in ("x", "y", "ret", "stats"):
            assert torch.equal(out[k], want[k]), k
        assert torch.equal(torch.nan_to_num(out["v"], nan=-1.0), torch.nan_to_num(want["v"], nan=-1.0))


def test_lapmod_solver():
    import lap
    from solvers import LAPMODSolver
    solver = LAPMODSolver()
    c = CASES["known8_dense"]
    D = densify(c)
    _, rx, _ = c["ref"][3]
    rows, cols, cost = solver.solve(D)
    assert cost == 17.0 == lap.get_cost(*problem(c), rx) and np.array_equal(cols, rx) and cols.dtype == np.int64
    assert np.array_equal(rows, np.arange(8))
    # masked: the 1000s become LARGE, which forces the rescaling to 999999
    _, mx, _ = CASES["known8_masked"]["ref"][3]
    rows, cols, cost = solver.solve(D, mask=D != 1000)
    assert cost == pytest.approx(17.0, rel=1e-9) and D[rows, cols].sum() == 17.0
    # costs of 1e6 and more are scaled down and the cost scaled back
    rows, cols, cost = solver(D * 1e6)
    assert cost == pytest.approx(17e6, rel=1e-9) and D[rows, cols].sum() == 17.0
    for fp in (lap.FP_1, lap.FP_2):
        assert solver.solve(D, fp_version=fp)[2] == 17.0
