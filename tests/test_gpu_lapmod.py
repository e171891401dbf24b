"""Sparse LAPMOD on the MI355X against the reference's lapmod_internal (tests/golden/lapmod_cases.npz): every case
for FP_1, FP_2 and FP_DYNAMIC through `lap.lapmod_sparse`, `lap.lapmod_many` and `WarmStartPipeline.lapmod_ragged`,
the final duals, the dense solver on the densified matrix, the stats, the LDS / workspace boundary, an unsolvable
instance inside a batch, graph capture, and `solvers.LAPMODSolver`."""
import numpy as np
import pytest

from host_common import shared_pipe as pipe  # noqa: F401
from lapmod_common import FP_VERSIONS, densify, load_cases, problem

pytestmark = pytest.mark.gpu

CASES, LDS_MAX = load_cases()
LABELS = list(CASES)


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
    assert checked >= 35


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
